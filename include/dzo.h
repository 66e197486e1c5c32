/*
 * dzo.h -- C ABI of the MI355X-native BFGS / L-BFGS step!() hot path.
 *
 * This is the drop-in boundary for dzhang314/DZOptimization.jl's in-place quasi-Newton
 * step.  The reference has NO FFI: its boundary is Julia multiple
 * dispatch on the array type parameter A<:AbstractArray{T} plus three user callbacks
 * (src/DZOptimization.jl:321-325,347-356).  A Julia host reaches this library with `ccall`
 * (dzoptimization.jl_amd/julia/DZOptimizationAMD.jl; INTEGRATION.md shows the binding); the
 * Python mirror used by the tests binds the same symbols with ctypes.
 *
 * Conventions
 *   - every function returns int32_t: 0 = DZO_OK, otherwise a DZO_ERR_* code;
 *     dzo_last_error() gives the message of the calling thread's last failure.  The
 *     reference signals only through @assert (AssertionError); those map to DZO_ERR_ASSERT.
 *   - plain pointers and sizes only.  `*_dev` pointers are device (HBM) addresses, everything
 *     else is host memory.  dtype is DZO_F32 or DZO_F64; scalars cross the ABI as double.
 *   - vectors are dense, contiguous, length n (N-d Julia arrays are treated linearly, as the
 *     reference does); matrices are n x n column-major (legacy/DZOptimization.jl:746).
 *   - one HIP stream per optimizer handle; calls on one handle must be serialised by the
 *     caller, different handles may be driven from different host threads (the reference's
 *     "independent optimizers" model, README.md:12).
 *   - asynchrony: step functions return as soon as the host-side decisions of the step are
 *     known; kernels that finish the step (delta_point, gradient, delta_gradient, rho) may still
 *     be running on the handle's stream.  Every getter (get_ptr, get_rho, ...) and
 *     dzo_synchronize() waits for them; touch an optimizer's device arrays from your own
 *     streams only after one of those, or enqueue on the handle's stream (dzo_lbfgs_stream).
 *   - there is no CPU fallback: every entry point needs the HIP device selected by dzo_init.
 *
 * All citations are file:line in the reference snapshot (2025-09-05).
 */
#ifndef DZO_H
#define DZO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DZO_VERSION 100 /* 0.1.0 */

/* element types (type parameter T of the reference's optimizers) */
#define DZO_F32 0
#define DZO_F64 1

/* status codes */
#define DZO_OK 0
#define DZO_ERR_INVALID 1     /* bad argument */
#define DZO_ERR_HIP 2         /* a HIP runtime call failed */
#define DZO_ERR_ASSERT 3      /* a reference @assert would have fired */
#define DZO_ERR_NOMEM 4
#define DZO_ERR_UNSUPPORTED 5
#define DZO_ERR_STATE 6       /* entry point called out of sequence */

/* built-in synthetic objectives; the reference's user callbacks */
#define DZO_PROBLEM_ROSENBROCK2D 0      /* legacy/ExampleFunctions.jl:10-24, README.md:25-31 */
#define DZO_PROBLEM_ROSENBROCK_CHAIN 1  /* sum 100(x[i+1]-x[i]^2)^2 + (1-x[i])^2 */
#define DZO_PROBLEM_QUADRATIC 2         /* 1/2 x'Ax, dense symmetric A */
#define DZO_PROBLEM_LSE 3               /* log sum exp(x) + lambda/2 |x-c|^2 */
#define DZO_PROBLEM_QUADRATIC_CHAIN 4   /* sum 1/2 (x[i+1]-x[i])^2 + lambda/2 (x[i]-1)^2: the large-n convex quadratic (tridiagonal Hessian) */
#define DZO_PROBLEM_PAIRWISE_LJ 5       /* n = 3N, point = [x(0..N) | y | z]: sum over pairs of lj_energy(r2), src/ExampleFunctions.jl (one
                                         * replicas[:, :, k] of scripts/MonteCarlo.jl:198) */

/* radial functions of the pairwise objective (the reference is generic over energy_function::F) */
#define DZO_RADIAL_LENNARD_JONES 0      /* lj_energy / lj_first_derivative / lj_second_derivative, src/ExampleFunctions.jl:16-72 */
/* The Morse pair term E(r) = t^2 - 2 t with t = exp(rho (1 - r)), r = sqrt(r2), in reduced units: the pair minimum is at r = 1
 * and its depth is 1.  first = dE/d(r2) = -rho t (t - 1) / r, second = d2E/d(r2)2 = rho t (rho r (2t - 1) + (t - 1)) / (2 r2 r).
 * rho is a compile-time constant of the kernels: one selector per range, every unit that takes `radial` takes these. */
#define DZO_RADIAL_MORSE_RHO6 2         /* (1 is not a selector) */
#define DZO_RADIAL_MORSE_RHO14 3

/* how compute_lbfgs_step_direction! is executed on the device */
#define DZO_TWOLOOP_CHAIN 0 /* 2k+1 fused axpy+dot links in the reference's op order */
#define DZO_TWOLOOP_GRAM 1  /* one Gram pass + O(k^2) scalar recurrence + one combine pass */

#define DZO_LINE_SEARCH_BACKTRACKING 0 /* take_backtracking_step! (src/DZOptimization.jl:107-154), the reference */
#define DZO_LINE_SEARCH_WOLFE 1        /* strong Wolfe on the LineSearchEvaluator quotients (:65-92) */

/* dense BFGS last_step_type (legacy/DZOptimization.jl:727-731) */
#define DZO_STEP_NULL 0
#define DZO_STEP_GRADIENT_DESCENT 1
#define DZO_STEP_BFGS 2

typedef struct dzo_problem_s *dzo_problem_t;
typedef struct dzo_lbfgs_s *dzo_lbfgs_t;
typedef struct dzo_adgd_s *dzo_adgd_t;
typedef struct dzo_bfgs_s *dzo_bfgs_t;
typedef struct dzo_bfgs_batch_s *dzo_bfgs_batch_t;
typedef struct dzo_comm_s *dzo_comm_t;

/* User callbacks, in the reference's order constraint / objective / gradient
 * (src/DZOptimization.jl:323-325).  They receive DEVICE pointers and must enqueue their
 * work on the stream returned by dzo_*_stream() or synchronise themselves.
 *   constraint_function!(x)::Bool  (:71-72,134-135)  -> nonzero = feasible; NULL = `nothing`
 *   objective_function(x)::T       (:80,138)         -> value as double
 *   gradient_function!(g, x)       (:87,479)         -> return ignored */
typedef int32_t (*dzo_constraint_fn)(void *ctx, void *x_dev);
typedef double (*dzo_objective_fn)(void *ctx, const void *x_dev);
typedef void (*dzo_gradient_fn)(void *ctx, void *g_dev, const void *x_dev);

/* ---------------------------------------------------------------------------------------
 * lifecycle
 * ------------------------------------------------------------------------------------- */
/* dzo_init selects `device` for the CALLING THREAD (hipSetDevice + the library's per-device context:
 * stream, scratch) and may be called for several devices; handle-less entry points (vector primitives,
 * dzo_malloc, constructors) work on the device the calling thread selected last.  dzo_memcpy_* find the
 * device from the pointer.  Optimizer handles other than the batched one must be driven with their
 * creating device selected. */
int32_t dzo_init(int32_t device);
int32_t dzo_shutdown(void);
int32_t dzo_version(void);
const char *dzo_last_error(void);
int32_t dzo_device_info(char *name, int32_t name_len, int32_t *compute_units, int64_t *hbm_bytes);
/* the number of HIP devices the process sees; needs no dzo_init (one shard per GPU from one process: dzo_comm_init_all) */
int32_t dzo_device_count(int32_t *count);
int32_t dzo_synchronize(void);

/* Per-kernel HIP-event timing on the launching stream (bench.py's roofline leg).
 * Entry i of the table is one kernel name with its launch count and total milliseconds. */
int32_t dzo_profile_enable(int32_t level); /* 0 off, 1 roofline kernels only, 2 every kernel */
int32_t dzo_profile_reset(void);
int32_t dzo_profile_count(int32_t *count);
int32_t dzo_profile_get(int32_t i, char *name, int32_t name_len, int64_t *launches, double *total_ms);

/* Diagnostic.  Kernels hand short results to the host (a trial's outcome, the line searches' state: what the reference
 * keeps in host scalars, src/DZOptimization.jl:328-335) through pinned memory: the result words, their SEAL (the xor of
 * their bits and of a ticket), then the ticket the host spins on.  The host reads the results only once the seal
 * matches: on MI355X it has been seen to read a new ticket next to the previous publish's words (1 to 5 times in
 * 10 000 waits when they lie in different cache lines).  *count = how often a wait had to look twice, process-wide. */
int32_t dzo_unsealed_first_reads(int64_t *count);

/* Calibration (SURVEY.md 8(d) "calibrate on the box"): GB/s of a plain read-only streaming kernel over
 * `bytes` of device memory re-read `repeats` times.  <= ~200 MiB stays in the Infinity Cache (the ceiling of
 * config 2, H = 128 MiB); several GiB give the HBM streaming ceiling. */
/* Self-test: the quotient the L-BFGS recurrence forms without a division (fd_div, csrc/dzo_lbfgs.hip) against a / b on the
 * device, `pairs` operand pairs of kind `mode` (0 random, 1 special divisors, 2 exact-ish quotients, 3 quotients next to a
 * rounding boundary, 4 small integers); *mismatches must come back 0.  first4: a, b, a / b, fd_div of the first mismatch. */
int32_t dzo_selftest_fast_div(uint64_t seed, int64_t pairs, int32_t mode, int64_t *checked, int64_t *mismatches, double *first4);
int32_t dzo_calibrate_read_bandwidth(int64_t bytes, int32_t repeats, double *gbps);
/* the same reader over a device buffer of the caller's, whatever it holds */
int32_t dzo_calibrate_read_bandwidth_of(const void *buf_dev, int64_t bytes, int32_t repeats, double *gbps);
/* GFLOP/s (2 per fma) of a register-only loop of `iters` x 16 independent fma chains per lane on every CU: the vector-ALU
 * ceiling the pairwise kernels below are measured against */
int32_t dzo_calibrate_fma_rate(int32_t dtype, int64_t iters, double *gflops);

/* ---------------------------------------------------------------------------------------
 * device memory (what `similar` / `copy` / `Array(x)` do for a GPU array type A)
 * ------------------------------------------------------------------------------------- */
int32_t dzo_malloc(void **ptr_dev, int64_t bytes);
int32_t dzo_free(void *ptr_dev);
int32_t dzo_memcpy_h2d(void *dst_dev, const void *src_host, int64_t bytes);
int32_t dzo_memcpy_d2h(void *dst_host, const void *src_dev, int64_t bytes);
int32_t dzo_memcpy_d2d(void *dst_dev, const void *src_dev, int64_t bytes);

/* ---------------------------------------------------------------------------------------
 * L1 vector primitives: the method set a Julia `HipVector{T}` needs so the
 * reference's generic code runs unmodified.  Blocking where they return a host scalar.
 * ------------------------------------------------------------------------------------- */
/* y += alpha*x            LinearAlgebra.axpy!  src/DZOptimization.jl:70,124,441,448 */
int32_t dzo_axpy(int64_t n, int32_t dtype, double alpha, const void *x_dev, void *y_dev);
/* y = alpha*x + beta*y    LinearAlgebra.axpby! src/DZOptimization.jl:145,308,480 */
int32_t dzo_axpby(int64_t n, int32_t dtype, double alpha, const void *x_dev, double beta, void *y_dev);
/* x *= alpha              LinearAlgebra.rmul!  src/DZOptimization.jl:387,444 */
int32_t dzo_scal(int64_t n, int32_t dtype, double alpha, void *x_dev);
/* dst = src               Base.copy!           src/DZOptimization.jl:69,118,151,306,386,438,478 */
int32_t dzo_copy(int64_t n, int32_t dtype, const void *src_dev, void *dst_dev);
/* x .= value              Base.fill!           src/DZOptimization.jl:222,227,369,374,384 */
int32_t dzo_fill(int64_t n, int32_t dtype, double value, void *x_dev);
/* x.y                     LinearAlgebra.dot    src/DZOptimization.jl:88,440,444,447,505 */
int32_t dzo_dot(int64_t n, int32_t dtype, const void *x_dev, const void *y_dev, double *result);
/* |x|_2                   LinearAlgebra.norm   src/DZOptimization.jl:230,292,294,381 */
int32_t dzo_nrm2(int64_t n, int32_t dtype, const void *x_dev, double *result);
/* isequal(a, b)           Base.isequal         src/DZOptimization.jl:128 (NaN==NaN, -0.0!=0.0) */
int32_t dzo_isequal(int64_t n, int32_t dtype, const void *a_dev, const void *b_dev, int32_t *result);
/* dst = t*d + x           out-of-place trial point, legacy/Kernels.jl:127-135,
 *                         legacy/DZOptimization.jl:33, src/DZOptimization.jl:69-70 */
int32_t dzo_trial_point(int64_t n, int32_t dtype, void *dst_dev, double t, const void *d_dev,
                        const void *x_dev);

/* The legacy primitives that have no LinearAlgebra twin above:
 *   norm2(x)            sum of squares -- NOT its square root     legacy/Kernels.jl:49-55,139
 *   inv_norm(x)         rsqrt(norm2(x))                           legacy/Kernels.jl:141
 *   negate!(x)          x[i] = -x[i]                              legacy/Kernels.jl:76-83,143
 *   scale!(dst, a, x)   dst[i] = a*x[i], out of place             legacy/Kernels.jl:96-104
 * (in-place scale! is dzo_scal, delta! is dzo_axpby(1, x, -1, y), both axpy! forms are dzo_axpy /
 * dzo_trial_point, dot is dzo_dot.) */
int32_t dzo_norm2(int64_t n, int32_t dtype, const void *x_dev, double *result);
int32_t dzo_inv_norm(int64_t n, int32_t dtype, const void *x_dev, double *result);
int32_t dzo_negate(int64_t n, int32_t dtype, void *x_dev);
int32_t dzo_scal_oop(int64_t n, int32_t dtype, void *dst_dev, double alpha, const void *x_dev);

/* ---------------------------------------------------------------------------------------
 * built-in objectives (device-side twins of the user's callbacks)
 * ------------------------------------------------------------------------------------- */
int32_t dzo_problem_create(int32_t kind, int64_t n, int32_t dtype, const void *A_dev,
                           const void *c_dev, double lambda, dzo_problem_t *out);
int32_t dzo_problem_destroy(dzo_problem_t p);
/* Decorators of legacy/DZOptimization.jl:219-296, applied on the device:
 *   set_l2            L2RegularizationWrapper (f + lambda*norm2(x), :231-232) and L2GradientWrapper
 *                     (g += 2*lambda*x, :241-249); lambda = 0 switches it off
 *   set_box_gradient  UniformBoxGradientWrapper (:282-296): g[i] = 0 where x[i] sits on a bound
 *                     and the gradient pushes outward
 *   set_box_constraint UniformBoxConstraint (:264-272) used as the optimizers' constraint_function!
 *                     (clamp, always feasible) when the optimizer is created from this problem */
int32_t dzo_problem_set_l2(dzo_problem_t p, double lambda);
int32_t dzo_problem_set_box_gradient(dzo_problem_t p, int32_t enable, double lower_bound, double upper_bound);
int32_t dzo_problem_set_box_constraint(dzo_problem_t p, int32_t enable, double lower_bound, double upper_bound);
/* x[i] = clamp(x[i], lo, hi)   UniformBoxConstraint call, legacy/DZOptimization.jl:264-272 */
int32_t dzo_box_clamp(int64_t n, int32_t dtype, void *x_dev, double lower_bound, double upper_bound);
int32_t dzo_problem_eval(dzo_problem_t p, const void *x_dev, double *f);
int32_t dzo_problem_grad(dzo_problem_t p, void *g_dev, const void *x_dev);
/* The built-in objectives in the SHAPE of the reference's three callbacks (src/DZOptimization.jl:323-325,
 * called at :134-138 and :479): pass these function pointers with ctx = the dzo_problem_t to
 * dzo_lbfgs_create_callbacks / dzo_adgd_set_callbacks and the optimizer runs its general (callback)
 * path on a device-side objective -- what a Julia host does when its callbacks are closures over
 * dzo_problem_eval / dzo_problem_grad, without a host-language frame in the loop.  The constraint
 * callback projects into the problem's box (legacy/DZOptimization.jl:264-272) when one is set and
 * reports the point feasible; an error inside a callback is reported as +Inf / a NaN-filled gradient
 * / infeasible, since the reference's callbacks have no error channel. */
double dzo_problem_objective_cb(void *problem, const void *x_dev);
void dzo_problem_gradient_cb(void *problem, void *g_dev, const void *x_dev);
int32_t dzo_problem_constraint_cb(void *problem, void *x_dev);

/* ---------------------------------------------------------------------------------------
 * pairwise radial N-body functions (src/ExampleFunctions.jl): the reference's own GPU kernels.
 * SoA coordinates x, y, z of n_particles particles, e = the radial function of r2 = |r_i - r_j|^2 selected by `radial`
 * (DZO_RADIAL_LENNARD_JONES, DZO_RADIAL_MORSE_RHO6, DZO_RADIAL_MORSE_RHO14).  Per pair the arithmetic is the reference's, operation by operation; the self term is removed
 * by a select.  Sums over j run in a fixed order (no floating-point atomics): the same input gives the same bits on every
 * call.  Blocking.  The pointers need no alignment beyond the element's.  Unknown radial, null pointers, i outside
 * 0 .. N-1: DZO_ERR_INVALID; a host pointer where the reference asserts get_backend equality: DZO_ERR_ASSERT.
 * DZO_PROBLEM_PAIRWISE_LJ is the same objective as a problem handle for the optimizers.
 * ------------------------------------------------------------------------------------- */
/* E = sum_i 1/2 sum_{j != i} e(r2_ij)      accelerated_pairwise_radial_energy + its kernel, :117-173 */
int32_t dzo_pairwise_energy(int32_t radial, int64_t n_particles, int32_t dtype,
                            const void *x_dev, const void *y_dev, const void *z_dev, double *energy);
/* g_i = 2 sum_{j != i} e'(r2_ij) (r_i - r_j)   accelerated_pairwise_radial_gradient! + its kernel, :224-294 */
int32_t dzo_pairwise_gradient(int32_t radial, int64_t n_particles, int32_t dtype,
                              void *gx_dev, void *gy_dev, void *gz_dev,
                              const void *x_dev, const void *y_dev, const void *z_dev);
/* p_i = 2 sum_{j != i} [ e' (u_i - u_j) + 2 (overlap e'') (r_i - r_j) ], overlap = (r_i - r_j).(u_i - u_j): the Hessian
 * applied to (u, v, w)                      accelerated_pairwise_radial_hvp! + its kernel, :367-468 */
int32_t dzo_pairwise_hvp(int32_t radial, int64_t n_particles, int32_t dtype,
                         void *px_dev, void *py_dev, void *pz_dev,
                         const void *x_dev, const void *y_dev, const void *z_dev,
                         const void *u_dev, const void *v_dev, const void *w_dev);
/* sum_{j != i} e(r2_new) - sum_{j != i} e(r2_old) for particle i (0-based) moved to (x_new, y_new, z_new): O(N), one
 * launch                                    pairwise_radial_energy_delta, :477-534 */
int32_t dzo_pairwise_energy_delta(int32_t radial, int64_t n_particles, int32_t dtype,
                                  const void *x_dev, const void *y_dev, const void *z_dev,
                                  int64_t i, double x_new, double y_new, double z_new, double *delta);

/* ---------------------------------------------------------------------------------------
 * Parallel-tempering Monte Carlo over replicas of one cluster (scripts/MonteCarlo.jl): the program pairwise_radial_energy_delta
 * was written for, with the loop over the moves on the device.  One launch runs num_steps Metropolis moves of every replica;
 * nothing crosses the host between moves.
 *
 * Layout.  replicas_dev is the reference's Array{T,3}(particles, 3, replicas) (:198): per replica [x(0..N) | y | z], 3N elements,
 * replica k at element 3N k -- one point of DZO_PROBLEM_PAIRWISE_LJ, so a replica can be handed to an optimizer.  The handle
 * ALIASES it (the reference mutates the caller's array).  energies_dev is (iterations, replicas) column-major with leading
 * dimension ld >= num_steps: energies[i + ld k].  A view of rows of a larger matrix (:223-224) is its first element + the ld
 * of the larger matrix.
 *
 * Launch shapes.  n_particles <= 64: one wave per replica, lane j holds particle j in registers.  65 .. 1024
 * (DZO_TEMPERING_MAX_PARTICLES): one 256-thread block per replica, coordinates in LDS.  More: DZO_ERR_UNSUPPORTED.
 *
 * Random numbers -- THE SPECIFICATION of what a temper / swap call computes.  Replica k owns one PCG32 (XSH-RR) stream, the
 * generator of legacy/PCG.jl:7-22:   advance(s) = 0x5851F42D4C957F2D s + 0x14057B7EF767814F (mod 2^64),
 *                                     extract(s) = rotr32(((s >> 18) ^ s) >> 27, s >> 59),
 * state after create = advance(0x14057B7EF767814F + base_seed + k); a draw is extract(state), then state = advance(state).
 * The 64-bit states live in device memory between calls (DZO_TEMPERING_RNG_STATES).
 * A Monte Carlo step consumes exactly SIX draws d0 .. d5, whatever branch it takes:
 *     j        = (d0 * N) >> 32                                   the particle, 0-based              (:49)
 *     u_i      = (d_i + 1/2) 2^-32 in fp64, i = 1 .. 4            (exact; never 0 or 1)
 *     n_x, n_y = sqrt(-2 log u_1) (cos, sin)(2 pi u_2), n_z = sqrt(-2 log u_3) cos(2 pi u_4) in fp64, each rounded to T
 *                (Box-Muller; the fourth normal is not used)                                          (:53-55)
 *     u        = d5 2^-32 in fp64 (exact), rounded to T: the acceptance uniform, in [0, 1]            (:63)
 * A swap decision consumes exactly ONE draw of the LOWER replica's stream (u as above), accepted or not   (:127)
 * Julia's own rand / randn streams cannot be reproduced and nothing here pretends to: a run is comparable with a Julia run
 * in distribution only.
 *
 * Arithmetic.  Proposal x_old + radius * n_x: a product and a sum, two roundings in T.  Sphere test x^2 + y^2 + z^2 < R^2 in T,
 * left to right.  Energy difference: per pair the operations of pairwise_radial_energy_delta; the sums over j in a fixed
 * order (lane sums in T, across lanes in fp64, one rounding back), no floating-point atomics: the same seed gives the same
 * bits.  Accept when delta <= 0 || u <= exp(-inv_temp * delta) (exp in T).
 *
 * Errors follow the pairwise functions: unknown radial, sizes < 1, null pointers DZO_ERR_INVALID; a host pointer where the
 * reference asserts that the axes / backends agree DZO_ERR_ASSERT.  temper, swap and run do NOT block (they enqueue on the
 * library's stream of the calling thread's device); read, analyze, dzo_synchronize and dzo_memcpy_* do.
 * ------------------------------------------------------------------------------------- */
#define DZO_TEMPERING_MAX_PARTICLES 1024
/* `what` of get_ptr / read / set: element type and count */
#define DZO_TEMPERING_REPLICAS 0        /* T, 3 N R: the caller's array */
#define DZO_TEMPERING_RADII 1           /* T, R: perturbation_radii (:13), adapted by every temper call; settable */
#define DZO_TEMPERING_INV_TEMPS 2       /* T, R: inverse_temperatures (:12) */
#define DZO_TEMPERING_NUM_ACCEPT 3      /* int64, R: num_accept of the last temper call (:46) */
#define DZO_TEMPERING_NUM_REJECT 4      /* int64, R: num_reject of the last temper call (:47) */
#define DZO_TEMPERING_RNG_STATES 5      /* uint64, R: the PCG32 states; settable (checkpoint / resume) */
#define DZO_TEMPERING_REC_INDEX 6       /* int32, (capacity, R): particle of step i of replica k at [i + capacity k] */
#define DZO_TEMPERING_REC_NORMALS 7     /* T, (3, capacity, R): n_x, n_y, n_z at [3 (i + capacity k) + c] */
#define DZO_TEMPERING_REC_UNIFORM 8     /* T, (capacity, R): the acceptance uniform */
#define DZO_TEMPERING_REC_CODE 9        /* int8, (capacity, R): 0 rejected by the Metropolis test, 1 accepted, 2 outside the sphere */
#define DZO_TEMPERING_REC_SWAP 10       /* int8, R: last swap call; slot a of a pair (a, a + 1): 1 exchanged, 0 not; other slots -1 */
#define DZO_TEMPERING_REC_SWAP_LOGP 11  /* T, R: log_prob of that pair (:126) in slot a; other slots 0 */
typedef struct dzo_tempering_s *dzo_tempering_t;
/* The arguments of parallel_temper! that outlive a call (:8-15).  inverse_temperatures and perturbation_radii are HOST arrays
 * of n_replicas doubles, rounded to T and kept on the device. */
int32_t dzo_tempering_create(int32_t radial, int64_t n_particles, int64_t n_replicas, int32_t dtype, void *replicas_dev,
                             const double *inverse_temperatures, const double *perturbation_radii, double constraining_radius,
                             uint64_t base_seed, dzo_tempering_t *out);
int32_t dzo_tempering_destroy(dzo_tempering_t h);
/* parallel_temper!, :8-86: the full energy of every replica, num_steps moves, energies[i, k] after every move, then the
 * radius adaptation of :77-81 (_fac = ten successive square roots of 2 in T).  energies_dev may be NULL (no trace). */
int32_t dzo_tempering_temper(dzo_tempering_t h, int64_t num_steps, void *energies_dev, int64_t ld);
/* parallel_swap!, :89-136: the pairs (a, a + 1), a = 0, 2, ... (odd = 0) or a = 1, 3, ... (odd != 0); both energies recomputed,
 * log_prob = (E_a - E_b)(beta_a - beta_b), exchanged when log_prob >= 0 || u <= exp(log_prob).  Coordinates move;
 * temperatures, radii and random streams stay with the slot. */
int32_t dzo_tempering_swap(dzo_tempering_t h, int32_t odd);
/* the body of main's loop, :222-231: per batch temper (rows 2 b S ..), swap(false), temper (rows (2 b + 1) S ..), swap(true),
 * S = num_steps; energies_dev holds 2 S num_batches rows.  Enqueued with no host wait in between. */
int32_t dzo_tempering_run(dzo_tempering_t h, int64_t num_steps, int64_t num_batches, void *energies_dev, int64_t ld);
/* analyze, :139-180: per replica the means V1, V2, V3 of E, E^2, E^3 over n_iterations rows (terms and sums in fp64, a fixed
 * order, one rounding to T), then cv and cv_prime by :173-176 in T.  Results to HOST arrays of doubles: cv[R], cv_prime[R],
 * moments[3 R] = (V1, V2, V3) per replica (moments may be NULL).  Blocking. */
int32_t dzo_tempering_analyze(dzo_tempering_t h, int64_t n_iterations, const void *energies_dev, int64_t ld, double *cv,
                              double *cv_prime, double *moments);
/* Record the draws and decisions of the temper calls that follow (up to capacity_steps steps per call; longer calls are
 * DZO_ERR_INVALID while recording) and of the swap calls; 0 switches recording off.  Every call overwrites the record. */
int32_t dzo_tempering_set_record(dzo_tempering_t h, int64_t capacity_steps);
/* device address of an array above (no wait) / a blocking copy of it to host memory / host memory copied into it (blocking;
 * DZO_TEMPERING_RADII and DZO_TEMPERING_RNG_STATES only).  Host arrays are in the array's own element type. */
int32_t dzo_tempering_get_ptr(dzo_tempering_t h, int32_t what, void **ptr_dev);
int32_t dzo_tempering_read(dzo_tempering_t h, int32_t what, void *out_host);
int32_t dzo_tempering_set(dzo_tempering_t h, int32_t what, const void *in_host);

/* ---------------------------------------------------------------------------------------
 * Batched LBFGSOptimizer over many small Lennard-Jones clusters (src/DZOptimization.jl:321-509 with constraint_function! =
 * nothing, objective = the pairwise radial energy above): the quench of the replicas that tempering leaves behind.  One
 * launch runs `steps` calls of step!() (:454-509) of EVERY instance; nothing crosses the host between steps or trials.
 *
 * Layout.  points_dev is (3N, batch): instance b at element 3N b, [x(0..N) | y | z] -- the tempering replica layout and one
 * point of DZO_PROBLEM_PAIRWISE_LJ.  The handle ALIASES it, like the live constructor aliases initial_point (:393): after a
 * step the caller's array holds the new points.
 *
 * Launch shapes.  n_particles <= 64: one wave per instance, lane i holds particle i, vectors in registers, the history in
 * LDS.  65 .. 1024 (DZO_LBFGS_BATCH_MAX_PARTICLES): one 256-thread block per instance, vectors in LDS; the history in LDS
 * where (2 history_length + 5) 3N elements fit the 160 KiB, else in device memory.  More: DZO_ERR_UNSUPPORTED.
 *
 * Arithmetic, per instance.  Constructor: f0, g0, first direction -initial_step_length g / |g|, is_stuck = iszero(|g0|)
 * (:381-387).  step!(): the two-loop recursion in its chain form over at most history_length pairs, newest first (:430-451;
 * rho holds s.y itself); take_backtracking_step! from t = 1 (:107-154): trial = fma(t, direction, old point), stuck when the
 * trial isequal the old point, accepted on strict decrease, halved otherwise; then delta_point = new - old, delta_gradient =
 * new - old by subtraction, the pair pushed first.  Energy and gradient of a trial come from one pair loop with the per-pair
 * operations of dzo_pairwise_* (a pair's value has the same bits); row sums over j = 0 .. N-1 in T, rows added in fp64 in a
 * fixed tree, one rounding to T; dots in fp64, fixed order, alpha / beta / the scale rounded to T.  The orders depend on N,
 * history_length and the element type only: an instance computes the same bits alone or anywhere in any batch.  No
 * floating-point atomics.  Deviation (as dzo_lbfgs_set_max_halvings): after max_halvings rejected trials (default 4096) the
 * instance is stuck.  A stuck instance does nothing more; on the step that finds it stuck delta_point keeps the copy of the
 * point made at :118 and delta_gradient is not touched, as in the reference.
 *
 * Errors follow the pairwise and tempering entries: unknown radial or dtype, sizes < 1, steps < 0, history_length < 1, null
 * pointers DZO_ERR_INVALID; n_particles > 1024 or history_length > 32 DZO_ERR_UNSUPPORTED; a host pointer where the reference
 * asserts backend equality (:363-364) DZO_ERR_ASSERT.  step enqueues on the library's stream and blocks only for all_stuck;
 * read and count_active block.
 * ------------------------------------------------------------------------------------- */
#define DZO_LBFGS_BATCH_MAX_PARTICLES 1024
#define DZO_LBFGS_BATCH_MAX_HISTORY   32
/* `what` of get_ptr / read: element type and shape (T = the handle's element type, m = history_length) */
#define DZO_LBFGS_BATCH_POINTS 0            /* T, 3N batch: the caller's array, current_point (:393) */
#define DZO_LBFGS_BATCH_GRADIENTS 1         /* T, 3N batch: current_gradient */
#define DZO_LBFGS_BATCH_DIRECTIONS 2        /* T, 3N batch: step_direction of the last step */
#define DZO_LBFGS_BATCH_DELTA_POINTS 3      /* T, 3N batch: delta_point */
#define DZO_LBFGS_BATCH_DELTA_GRADIENTS 4   /* T, 3N batch: delta_gradient */
#define DZO_LBFGS_BATCH_OBJECTIVES 5        /* T, batch: current_objective_value */
#define DZO_LBFGS_BATCH_DELTA_OBJECTIVES 6  /* T, batch: delta_objective_value */
#define DZO_LBFGS_BATCH_IS_STUCK 7          /* int32, batch */
#define DZO_LBFGS_BATCH_ITERATION_COUNTS 8  /* int64, batch */
#define DZO_LBFGS_BATCH_HISTORY_COUNTS 9    /* int32, batch: pairs held, <= m */
#define DZO_LBFGS_BATCH_S 10                /* T, (3N, m, batch): delta_point_history, newest first; pair k of instance b at 3N (k + m b) */
#define DZO_LBFGS_BATCH_Y 11                /* T, (3N, m, batch): delta_gradient_history, newest first */
#define DZO_LBFGS_BATCH_RHO 12              /* fp64, (m, batch): rho_history = s.y, newest first */
#define DZO_LBFGS_BATCH_LAST_HALVINGS 13    /* int32, batch: h of the last accepted step (t = 2^-h); on a stuck step the halvings tried */
typedef struct dzo_lbfgs_batch_s *dzo_lbfgs_batch_t;
/* LBFGSOptimizer(nothing, f, g!, initial_point, initial_step_length, history_length) of every instance, :400-427 and :347-397.
 * points_dev: (3N, batch), instance b at element 3N b, [x | y | z] -- the tempering replica layout; ALIASED like the live
 * constructor aliases initial_point (:393).  initial_step_length <= 0: DZO_ERR_ASSERT (:380).  Blocking. */
int32_t dzo_lbfgs_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                               double initial_step_length, int32_t history_length, dzo_lbfgs_batch_t *out);
int32_t dzo_lbfgs_batch_destroy(dzo_lbfgs_batch_t h);
/* the bound on the halvings of one step (the loop of :121-153 has none); at least 1 */
int32_t dzo_lbfgs_batch_set_max_halvings(dzo_lbfgs_batch_t h, int64_t max_halvings);
/* `steps` step!() calls (:454-509) of every instance that is not stuck, one launch; all_stuck may be NULL (then no host wait) */
int32_t dzo_lbfgs_batch_step(dzo_lbfgs_batch_t h, int32_t steps, int32_t *all_stuck);
/* instances with is_stuck == false (:456).  Blocking. */
int32_t dzo_lbfgs_batch_count_active(dzo_lbfgs_batch_t h, int64_t *active);
/* device address of an array above (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_lbfgs_batch_get_ptr(dzo_lbfgs_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_lbfgs_batch_read(dzo_lbfgs_batch_t h, int32_t what, void *out_host);
/* objective_function and gradient_function! (:416-421) of every instance: energy (T, batch) and, unless NULL, gradient
 * (T, 3N batch) of every instance of points_dev, by the SAME device routine and summation order the optimizer uses.
 * Blocking. */
int32_t dzo_pairwise_batch_energy_gradient(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype,
                                           const void *points_dev, void *energies_dev, void *gradients_dev);

/* ---------------------------------------------------------------------------------------
 * The Thomson problem: Riesz energy on the unit sphere and the sphere-constrained batched LBFGSOptimizer.  The objective is
 * the reference author's example of legacy/ExampleFunctions.jl, the Riesz (Coulomb, s = 1) energy of N points:
 *   riesz_energy                      :30-45     E = sum_{i < j} 1 / |p_i - p_j|
 *   riesz_gradient!                   :47-83     g_j = sum_{i != j} (p_i - p_j) / |p_i - p_j|^3, i ascending, the self term skipped
 *   constrain_riesz_gradient_sphere!  :361-374   g_i -= (p_i . g_i) p_i
 * and the optimizer is the live LBFGSOptimizer (src/DZOptimization.jl:321-509) WITH its constraint hook: the short constructor
 * projects the initial point (:412-414) and take_backtracking_step! projects every trial point before it is evaluated
 * (:133-135).  The sibling of dzo_lbfgs_batch_* above, whose constraint_function! is nothing: many random configurations of N
 * charges, each quenched to a local minimum in one launch.
 *
 * Layout.  points_dev is (3N, batch): instance b at element 3N b, [x(0..N) | y | z], the layout of every cluster unit.  (The
 * legacy functions take a (3, N) matrix; particle i here is column i there.)
 *
 * Arithmetic.  Per pair, from r2 = dx^2 + dy^2 + dz^2 summed in that order: r = sqrt(r2), inv_r = 1 / r (IEEE), energy inv_r,
 * gradient term 2 (-0.5 (inv_r / r2)) (p_i - p_j); inv_r / r2 is the reference's inv_dist_cubed (:62), the scaling by 1/2 and the
 * doubling are exact, so a term has the bits of the reference's dist * inv_dist_cubed, and a row is summed over j ascending like
 * :55-80.  E is half the sum over ordered pairs: row sums in T, rows added in fp64 in the fixed trees of dzo_lbfgs_batch_*, one
 * rounding to T.
 *   project(x, y, z):  r = sqrt(x^2 + y^2 + z^2) summed in that order, then x / r, y / r, z / r (IEEE divisions).  It always
 *       reports success; a particle on the origin becomes NaN, its objective NaN, and the trial is rejected (the step backtracks),
 *       which is what the reference does with a NaN objective.  The reference ships the gradient constraint but NOT the
 *       projection (constraint_function! is the caller's): per-particle normalisation is ours.
 *   tangent(p, g):     overlap = x gx + y gy + z gz summed in that order, unfused; g -= overlap p, unfused
 *       (constrain_riesz_gradient_sphere!, operation for operation).
 * Inside a trial (:124-139): trial = fma(t, direction, old point); stuck when the UNPROJECTED trial isequal the old point (:128);
 * project (:133-135); evaluate; make the trial's gradient tangent; accept on strict decrease.  On acceptance delta_point is
 * projected-new minus old and delta_gradient the difference of tangent gradients.  Everything else -- the constructor's first
 * direction (:381-387, on the tangent gradient of the projected initial point), the recursion (:430-451), the ring, the launch
 * shapes, determinism, max_halvings, errors and blocking rules -- is that of dzo_lbfgs_batch_*, with its `what` constants
 * (DZO_LBFGS_BATCH_*) and limits (DZO_LBFGS_BATCH_MAX_PARTICLES, DZO_LBFGS_BATCH_MAX_HISTORY).
 * ------------------------------------------------------------------------------------- */
#define DZO_SPHERE_ENERGY_RIESZ1 0          /* the only `energy` selector; anything else is DZO_ERR_INVALID */
/* constraint_function! (:133-135, :412-414) of every particle of every instance, in place: project above.  Blocking. */
int32_t dzo_sphere_batch_project(int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev);
/* riesz_energy (:30-45) into energies_dev (T, batch) and, unless NULL, riesz_gradient! (:47-83) into gradients_dev (T, 3N batch):
 * raw when tangent == 0, after constrain_riesz_gradient_sphere! (:361-374) when tangent == 1, by the SAME device routine and
 * summation order the optimizer uses.  The points are taken as they are (not projected).  Blocking. */
int32_t dzo_sphere_batch_energy_gradient(int32_t energy, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                         void *energies_dev, void *gradients_dev, int32_t tangent);
typedef struct dzo_sphere_lbfgs_batch_s *dzo_sphere_lbfgs_batch_t;
/* LBFGSOptimizer(constraint_function!, f, g!, initial_point, initial_step_length, history_length) of every instance, :400-427
 * and :347-397: points_dev is ALIASED (:393) and PROJECTED IN PLACE (:412-414), then f0, the tangent g0, the first direction and
 * is_stuck = iszero(|g0|) (:381-387).  `energy` sits where dzo_lbfgs_batch_create takes `radial`.  Blocking. */
int32_t dzo_sphere_lbfgs_batch_create(int32_t energy, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                      double initial_step_length, int32_t history_length, dzo_sphere_lbfgs_batch_t *out);
int32_t dzo_sphere_lbfgs_batch_destroy(dzo_sphere_lbfgs_batch_t h);
/* the bound on the halvings of one step (the loop of :121-153 has none); at least 1 */
int32_t dzo_sphere_lbfgs_batch_set_max_halvings(dzo_sphere_lbfgs_batch_t h, int64_t max_halvings);
/* `steps` step!() calls (:454-509) of every instance that is not stuck, one launch; all_stuck may be NULL (then no host wait) */
int32_t dzo_sphere_lbfgs_batch_step(dzo_sphere_lbfgs_batch_t h, int32_t steps, int32_t *all_stuck);
/* instances with is_stuck == false (:456).  Blocking. */
int32_t dzo_sphere_lbfgs_batch_count_active(dzo_sphere_lbfgs_batch_t h, int64_t *active);
/* device address of a DZO_LBFGS_BATCH_* array (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_sphere_lbfgs_batch_get_ptr(dzo_sphere_lbfgs_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_sphere_lbfgs_batch_read(dzo_sphere_lbfgs_batch_t h, int32_t what, void *out_host);

/* ---------------------------------------------------------------------------------------
 * Batched basin hopping over Lennard-Jones clusters (Wales & Doye 1997): Monte Carlo over the QUENCHED landscape, the
 * composition of the tempering move (scripts/MonteCarlo.jl:49-55, applied to every particle), the quench above
 * (src/DZOptimization.jl:321-509) and the Metropolis test (scripts/MonteCarlo.jl:63-70) on the quenched energies.  Each walker
 * is an instance of the batch.  One launch runs num_hops hops of EVERY walker at the walker's own pace; nothing crosses the
 * host between hops, and no walker waits for another's quench.
 *
 * Layout.  points_dev is the quench's (3N, batch): walker b at element 3N b, [x(0..N) | y | z].  The handle ALIASES it; it
 * always holds the walkers' current minima.
 *
 * Launch shapes.  n_particles <= 64: one wave per walker, lane i holds particle i; current minimum and quench state in
 * registers, the history ring in LDS.  65 .. 1024 (DZO_BASIN_HOPPING_MAX_PARTICLES): one 256-thread block per walker; the five
 * quench vectors plus the current minimum in LDS, the ring in LDS where (2 history_length + 6) 3N elements and the scalars
 * (16 history_length + 64 bytes) fit 159 KiB, else in device memory.  More: DZO_ERR_UNSUPPORTED.
 *
 * THE SPECIFICATION of what create and a hop compute.
 *   create   rounds inverse_temperatures and perturbation_radii to T and seeds walker b's PCG32 stream as tempering does:
 *            state = advance(0x14057B7EF767814F + base_seed + b).  It then enqueues the quench (below) of the caller's points.
 *            That quench consumes no draws, is always kept, and sets ENERGIES and BEST_*; it is not counted in
 *            QUENCH_ITERATIONS / QUENCH_UNFINISHED.  create does not wait for it.
 *   a hop    of walker b starts from stream state s and always consumes exactly 4N + 1 draws, whatever it decides: the
 *            state afterwards is pcg_jump(s, 4N + 1), s' = A_k s + C_k (the LCG skip).
 *            Particle i takes draws 4i .. 4i+3 as d1 .. d4 of the tempering rule and makes n_x, n_y, n_z by its formulas: fp64
 *            Box-Muller, each normal rounded to T, the fourth normal unused.  Draw 4N is the acceptance uniform
 *            u = d 2^-32, rounded to T.
 *            The trial coordinate is old + radius * n: a product and a sum in T.  A particle whose trial position fails
 *            x^2 + y^2 + z^2 < R^2 (in T, left to right; R = constraining_radius rounded to T) keeps its old position in the
 *            trial.
 *   quench   is exactly dzo_lbfgs_batch_create on the trial (initial_step_length, history_length) followed by
 *            dzo_lbfgs_batch_step(quench_steps) under the handle's max_halvings: the quenched point, its energy E_q, the
 *            iteration count and is_stuck have the bits of those calls.
 *   decision delta = E_q - E in T.  Accept iff E_q is finite and (delta <= 0 || u <= exp(-beta * delta)), exp in T.  On
 *            acceptance the quenched point and E_q become the walker's.  BEST_* is replaced whenever E_q is finite and
 *            E_q < BEST_ENERGY, accepted or not.  A start whose energy is not a number (two coincident particles) keeps
 *            that energy: every comparison with it is false, so no hop is accepted and BEST_* never changes; a quench
 *            that ends at a non-finite energy is code 2.
 *   adapt    when adapt != 0, at the end of the call the radius follows scripts/MonteCarlo.jl:77-81 on this call's counts,
 *            with the same _fac (ten successive square roots of 2 in T) and the same cap of 1.  When adapt == 0 the radii
 *            stay.
 * Reproducibility.  No floating-point atomics.  A walker computes the same bits alone or anywhere in any batch.  hop(a)
 * followed by hop(b) equals hop(a + b) when adapt == 0.
 *
 * Errors follow the quench and tempering entries: unknown radial or dtype, sizes < 1, quench_steps < 1, history_length < 1,
 * a constraining_radius that is not > 0, num_hops < 0, null pointers, a record capacity smaller than num_hops while recording
 * DZO_ERR_INVALID; n_particles > 1024 or history_length > 32 DZO_ERR_UNSUPPORTED; a host pointer for points_dev, or
 * initial_step_length <= 0, DZO_ERR_ASSERT (:363-364, :380).  create and hop enqueue on the library's stream and do not
 * block; read, set and set_record do.  A launch lasts num_hops quenches of its slowest walker: keep num_hops small (a
 * handful) and call again, so that the device stays responsive.
 * ------------------------------------------------------------------------------------- */
#define DZO_BASIN_HOPPING_MAX_PARTICLES 1024
/* `what` of get_ptr / read / set: element type and shape (T = the handle's element type) */
#define DZO_BASIN_HOPPING_POINTS 0                  /* T, 3N batch: the caller's array, the current minima */
#define DZO_BASIN_HOPPING_ENERGIES 1                /* T, batch: their energies */
#define DZO_BASIN_HOPPING_BEST_POINTS 2             /* T, 3N batch, handle-owned: the lowest minimum each walker has quenched to */
#define DZO_BASIN_HOPPING_BEST_ENERGIES 3           /* T, batch */
#define DZO_BASIN_HOPPING_RADII 4                   /* T, batch: perturbation radii; settable */
#define DZO_BASIN_HOPPING_INV_TEMPS 5               /* T, batch */
#define DZO_BASIN_HOPPING_NUM_ACCEPT 6              /* int64, batch: of the last hop call */
#define DZO_BASIN_HOPPING_NUM_REJECT 7              /* int64, batch: of the last hop call (codes 0 and 2) */
#define DZO_BASIN_HOPPING_RNG_STATES 8              /* uint64, batch: the PCG32 states; settable (checkpoint / resume) */
#define DZO_BASIN_HOPPING_HOP_COUNTS 9              /* int64, batch: hops since create */
#define DZO_BASIN_HOPPING_QUENCH_ITERATIONS 10      /* int64, batch: L-BFGS iterations of all hops since create */
#define DZO_BASIN_HOPPING_QUENCH_UNFINISHED 11      /* int64, batch: quenches of hops that ended not stuck */
#define DZO_BASIN_HOPPING_REC_NORMALS 12            /* T, (3, N, capacity, batch): n_x, n_y, n_z of particle p of hop i at [3 (p + N (i + capacity b)) + c] */
#define DZO_BASIN_HOPPING_REC_UNIFORM 13            /* T, (capacity, batch): the acceptance uniform */
#define DZO_BASIN_HOPPING_REC_TRIAL_ENERGY 14       /* T, (capacity, batch): E_q */
#define DZO_BASIN_HOPPING_REC_QUENCH_ITERATIONS 15  /* int32, (capacity, batch) */
#define DZO_BASIN_HOPPING_REC_CODE 16               /* int8, (capacity, batch): 0 rejected by the Metropolis test, 1 accepted, 2 rejected because the quenched energy is not finite */
typedef struct dzo_basin_hopping_s *dzo_basin_hopping_t;
/* inverse_temperatures and perturbation_radii are HOST arrays of batch doubles.  constraining_radius > 0, may be infinite. */
int32_t dzo_basin_hopping_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                 const double *inverse_temperatures, const double *perturbation_radii,
                                 double constraining_radius, double initial_step_length, int32_t history_length,
                                 int32_t quench_steps, uint64_t base_seed, dzo_basin_hopping_t *out);
int32_t dzo_basin_hopping_destroy(dzo_basin_hopping_t h);
/* the bound on the halvings of one quench step, as dzo_lbfgs_batch_set_max_halvings (default 4096); at least 1 */
int32_t dzo_basin_hopping_set_max_halvings(dzo_basin_hopping_t h, int64_t max_halvings);
/* num_hops hops of every walker, one launch; enqueues, does not block */
int32_t dzo_basin_hopping_hop(dzo_basin_hopping_t h, int64_t num_hops, int32_t adapt);
/* Record the draws and decisions of the hop calls that follow (up to capacity_hops hops per call; longer calls are
 * DZO_ERR_INVALID while recording); 0 switches recording off.  Every call overwrites the record from hop 0. */
int32_t dzo_basin_hopping_set_record(dzo_basin_hopping_t h, int64_t capacity_hops);
/* device address of an array above (no wait) / a blocking copy of it to host memory / host memory copied into it (blocking;
 * DZO_BASIN_HOPPING_RADII and DZO_BASIN_HOPPING_RNG_STATES only).  Host arrays are in the array's own element type.
 * Checkpoint / resume: read POINTS, RADII and RNG_STATES; create a handle at those points and set the two arrays.  A walker
 * goes on identically where the constructor's quench leaves its point as it is (a minimum found in fp64 does; in fp32 a stuck
 * point can still move by a decrease at rounding level, and the walker goes on from there). */
int32_t dzo_basin_hopping_get_ptr(dzo_basin_hopping_t h, int32_t what, void **ptr_dev);
int32_t dzo_basin_hopping_read(dzo_basin_hopping_t h, int32_t what, void *out_host);
int32_t dzo_basin_hopping_set(dzo_basin_hopping_t h, int32_t what, const void *in_host);

/* ---------------------------------------------------------------------------------------
 * Batched AdGDOptimizer over many small Lennard-Jones clusters (src/DZOptimization.jl:179-312 with constraint_function! =
 * nothing, objective = the pairwise radial energy above): the sibling of dzo_lbfgs_batch_* without a history ring.  One
 * launch runs `steps` calls of step!() (:274-312) of EVERY instance; nothing crosses the host between steps or trials.
 * Layout, launch shapes (one wave per instance up to 64 particles, one 256-thread block up to
 * DZO_ADGD_BATCH_MAX_PARTICLES), determinism, error codes and blocking rules are those of dzo_lbfgs_batch_*.
 *
 * Arithmetic, per instance (T = the element type).
 * Constructor (:229-241): f0 and g0 by the routine of dzo_pairwise_batch_energy_gradient; ss = g0.g0 in fp64; is_stuck =
 * (ss == 0); current_step_size = previous_step_size = is_stuck ? 0 : T(initial_step_length) / T(sqrt(ss)) (the norm rounded
 * to T, the division in T); delta_point, delta_gradient and delta_objective zero, iteration_count 0.
 * step!() (:274-312): a stuck instance does nothing.  With iteration_count > 0, every operation in T with IEEE division and
 * square root: theta = current / previous; next = current sqrt(1 + theta); dgn = sqrt(T(sum delta_gradient^2 in fp64)); if
 * dgn != 0: inv_L = sqrt(T(sum delta_point^2 in fp64)) / dgn and next = min(next, sqrt(T(1/2)) inv_L) -- the rule and the
 * operation order of dzo_adgd_*.  Else next = current.  Then previous = current, current = next (:298-299): before the search,
 * so also on a step that ends stuck.
 * take_backtracking_step!(opt, -next, current_gradient) (:107-154) from h = 0: trial = fma(-(next 2^-h), gradient, old point),
 * one fused multiply-add per element (the step is halved once per rejected trial); stuck when the trial isequal the old point
 * (:128); accepted on strict decrease (:139), otherwise h += 1.  Deviation (as dzo_lbfgs_set_max_halvings): after max_halvings
 * rejected trials (default 4096) the instance is stuck.
 * On acceptance: delta_objective = f_new - f, delta_point = new - old and delta_gradient = g_new - g by subtraction
 * (:306-308), iteration_count += 1.  The gradient of the accepted trial is kept: it is the value gradient_function! returns at
 * :307.  On the step that finds the instance stuck: the point is unchanged, delta_point holds the copy of the old point made
 * at :118, delta_gradient, f, g and iteration_count are untouched, and LAST_HALVINGS is the number of halvings tried.
 * Energy and gradient of a trial come from ONE pair loop, the optimizer's own device routine: the stored f and g of a handle
 * are, bit for bit, what dzo_pairwise_batch_energy_gradient returns for the stored points.  Sums of squares are in fp64 in a
 * fixed order that depends on N only.  No floating-point atomics.  An instance computes the same
 * bits alone or anywhere in any batch, and in one launch of k steps or k launches of one.
 *
 * Errors are those of dzo_lbfgs_batch_create: unknown radial or dtype, sizes < 1, steps < 0, null pointers, unknown `what`,
 * max_halvings < 1 DZO_ERR_INVALID; n_particles > 1024 DZO_ERR_UNSUPPORTED; a host pointer where the reference asserts
 * backend equality (:216-217) or initial_step_length <= 0 (:229) DZO_ERR_ASSERT.  create, read and count_active block; step
 * enqueues on the library's stream and blocks only for all_stuck.
 * ------------------------------------------------------------------------------------- */
#define DZO_ADGD_BATCH_MAX_PARTICLES 1024
/* `what` of get_ptr / read (T = the handle's element type) */
#define DZO_ADGD_BATCH_POINTS 0              /* T, 3N batch: the caller's array, current_point (aliased, :238) */
#define DZO_ADGD_BATCH_GRADIENTS 1           /* T, 3N batch: current_gradient */
#define DZO_ADGD_BATCH_DELTA_POINTS 2        /* T, 3N batch: delta_point */
#define DZO_ADGD_BATCH_DELTA_GRADIENTS 3     /* T, 3N batch: delta_gradient */
#define DZO_ADGD_BATCH_OBJECTIVES 4          /* T, batch: current_objective_value */
#define DZO_ADGD_BATCH_DELTA_OBJECTIVES 5    /* T, batch: delta_objective_value */
#define DZO_ADGD_BATCH_IS_STUCK 6            /* int32, batch */
#define DZO_ADGD_BATCH_ITERATION_COUNTS 7    /* int64, batch */
#define DZO_ADGD_BATCH_CURRENT_STEP_SIZES 8  /* T, batch: current_step_size (:195) */
#define DZO_ADGD_BATCH_PREVIOUS_STEP_SIZES 9 /* T, batch: previous_step_size (:196) */
#define DZO_ADGD_BATCH_LAST_HALVINGS 10      /* int32, batch: h of the last accepted step (step = -current_step_size 2^-h); on a stuck step the halvings tried */
typedef struct dzo_adgd_batch_s *dzo_adgd_batch_t;
/* AdGDOptimizer(nothing, f, g!, initial_point, initial_step_length) of every instance, :245-271 and :201-242.  points_dev:
 * (3N, batch), instance b at element 3N b, [x | y | z] -- the tempering replica layout; ALIASED like the live constructor
 * aliases initial_point (:238).  initial_step_length <= 0: DZO_ERR_ASSERT (:229).  Blocking. */
int32_t dzo_adgd_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                              double initial_step_length, dzo_adgd_batch_t *out);
int32_t dzo_adgd_batch_destroy(dzo_adgd_batch_t h);
/* the bound on the halvings of one step (the loop of :121-153 has none); default 4096, at least 1 */
int32_t dzo_adgd_batch_set_max_halvings(dzo_adgd_batch_t h, int64_t max_halvings);
/* `steps` step!() calls (:274-312) of every instance that is not stuck, one launch; all_stuck may be NULL (then no host wait) */
int32_t dzo_adgd_batch_step(dzo_adgd_batch_t h, int32_t steps, int32_t *all_stuck);
/* instances with is_stuck == false (:276).  Blocking. */
int32_t dzo_adgd_batch_count_active(dzo_adgd_batch_t h, int64_t *active);
/* device address of an array above (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_adgd_batch_get_ptr(dzo_adgd_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_adgd_batch_read(dzo_adgd_batch_t h, int32_t what, void *out_host);

/* ---------------------------------------------------------------------------------------
 * Batched Hessian-vector products and dense Hessians of many small Lennard-Jones clusters: second-order information on the
 * points the batched optimizers above leave behind (minimum or saddle, normal modes, curvature along a direction).  The
 * product is accelerated_pairwise_radial_hvp! (src/ExampleFunctions.jl:367-468) with lj_first_derivative and
 * lj_second_derivative (:50-72), every instance in ONE launch.  Both entry points block.
 *
 * Layout.  points, directions and products are (3N, batch): instance b at element 3N b, [x(0..N) | y | z] -- the tempering and
 * quench layout.  point_stride is the distance in elements between the points of consecutive instances: 3N (or more) for one
 * point per instance, 0 to apply `batch` directions to ONE point (a block product of one cluster); any other value below 3N is
 * DZO_ERR_INVALID.  curvatures_dev may be NULL; otherwise fp64, (2, batch): u.Hu at 2 b and u.u at 2 b + 1 (their quotient is
 * the Rayleigh quotient of direction b).  hessians are (3N, 3N, batch), column-major per instance like every matrix in this
 * header: element r + 3N (c + 3N b) is row r, column c of instance b; row a N + i is component a of particle i.
 *
 * Launch shapes.  n_particles <= 64: one wave per instance, lane i holds particle i (and its direction) in registers, particle j
 * arrives through a lane read, four independent pairs per trip, no barrier.  65 .. 1024 (DZO_HESSIAN_BATCH_MAX_PARTICLES): one
 * 256-thread block per instance, thread t owns particles t + 256 q, point and direction staged in LDS.
 *
 * Arithmetic (T = the element type; this is the specification).
 * Per pair (i, j), the body of :395-419 with the per-pair operations of dzo_pairwise_hvp, one rounding per operation:
 * d = r_i - r_j, du = u_i - u_j, r2 = dx dx + dy dy + dz dz (left to right), f = lj_first_derivative(r2) (:30-47), s =
 * lj_second_derivative(r2) (:50-72), overlap = dx du + dy dv + dz dw (left to right), g = twice(overlap s), term_a = f du_a +
 * g d_a.  The self term and the padding of the unrolled loop are computed and dropped by a select (f = s = 0; ifelse, :145).
 * The row sum of particle i runs j = 0 .. N-1 sequentially in T from +0; products_i = twice(sum) (:421-423).
 * u.Hu and u.u: an fp64 dot in a fixed order that depends on N only -- per particle u_x p_x, then fma(u_y, p_y, .), then
 * fma(u_z, p_z, .); N <= 64: the wave tree over the particles; above: a thread's particles t, t + 256, ... added in that order,
 * the wave tree, then the block's four wave sums in wave order.
 * Dense Hessian.  For finite inputs with no coincident particles, column c of hessians[b] has the same values as
 * dzo_pairwise_batch_hvp of points[b] with the unit direction e_c (compare with ==; the sign of a zero is free).  It is not
 * obtained by 3N products but assembled from one pass over the pairs: an off-diagonal block (i != j) is the single term with
 * du = -e_b: overlap = -d_b, g = twice(overlap s), entry (a, b) = twice(f du_a + g d_a); the diagonal block of particle i is the
 * sequential sum over j of f delta_ab + twice(d_b s) d_a, then twice.  All other terms of those product rows are exact zeros,
 * which is why the two agree.  Bitwise symmetry is NOT promised: (d_b s) d_a and (d_a s) d_b round differently.
 * No floating-point atomics: every element is written once by one thread.  An instance computes the same bits alone or anywhere
 * in any batch, and with point_stride 0 or 3N.  Coincident particles give non-finite values in their rows, as in the reference.
 *
 * Errors are those of dzo_pairwise_batch_energy_gradient: unknown radial or dtype, sizes < 1, a bad point_stride, null pointers
 * (curvatures_dev excepted) DZO_ERR_INVALID; n_particles > 1024 DZO_ERR_UNSUPPORTED; a host pointer where the reference asserts
 * backend equality (:453-461) DZO_ERR_ASSERT.
 * ------------------------------------------------------------------------------------- */
#define DZO_HESSIAN_BATCH_MAX_PARTICLES 1024
/* products[b] = Hessian(points[b]) applied to directions[b]     (:367-468, batched) */
int32_t dzo_pairwise_batch_hvp(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype,
                               const void *points_dev, int64_t point_stride,
                               const void *directions_dev, void *products_dev, double *curvatures_dev);
/* hessians[b] = the dense 3N x 3N Hessian of points[b] */
int32_t dzo_pairwise_batch_hessian(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype,
                                   const void *points_dev, void *hessians_dev);

/* ---------------------------------------------------------------------------------------
 * Batched symmetric eigensolver: the spectrum of many small dense symmetric matrices on the device -- the Hessians that
 * dzo_pairwise_batch_hessian writes, diagonalised where they are (minimum or saddle, the Morse index, the six rigid-body
 * zeros, normal modes).  Two-sided cyclic Jacobi in a parallel (round-robin) ordering, every instance in ONE launch, one
 * 256-thread block per instance.  Nothing in the reference diagonalises anything: this block is the specification.
 *
 * Layout.  matrices are (n, n, batch), column-major per instance like every matrix in this header: element r + n (c + n b) is
 * row r, column c of instance b.  eigenvalues are (n, batch), ascending.  eigenvectors are (n, n, batch), column-major: column k
 * of instance b belongs to eigenvalue k.  sweeps are int32, (batch).
 *
 * Storage (dzo_symeig_plan tells).  DZO_SYMEIG_STORAGE_LDS whenever 64 bytes, 2 m elements (m = n + (n & 1)) and n ld elements,
 * ld = n | 1 (the smallest odd number >= n), fit the 160 KiB of LDS of a compute unit: the matrix stays in LDS for the whole
 * iteration.  That covers n = 141 in fp64 (114 = 3 * 38 is the workload) and n = 201 in fp32.  Above that
 * DZO_SYMEIG_STORAGE_MEMORY: the same kernel body on a per-call device workspace copy with ld = n, functional rather than
 * fast, up to DZO_SYMEIG_MAX_N.  Both storages compute the same bits.  V lives in eigenvectors_dev in both.
 *
 * Arithmetic (T = the element type; every operation in T with one rounding, no contraction, IEEE division and square root,
 * unless fp64 is named).
 * 1. Load.  a[r,c] = T(0.5) * (A[r,c] + A[c,r]): the symmetric part (the Hessian kernel does not promise bitwise symmetry).
 *    With eigenvectors V = I.  fro = sqrt(sum a[r,c]^2), in fp64 in a fixed order that depends on n only, the ORDER OF THE
 *    NORMS: thread (w, l), w = 0 .. 3, l = 0 .. 63, adds the squares (one fp64 product, one fp64 sum each, from +0) of columns
 *    c = w, w + 4, ... (outer) and rows r = l, l + 64, ... (inner); the 64 values of a wave are added by the xor tree with
 *    offsets 32, 16, 8, 4, 2, 1; the four wave sums are added in wave order from +0.
 * 2. Sweep test, at the start of every sweep.  off = sqrt(sum over r != c of a[r,c]^2), from the off-diagonal entries
 *    themselves (never as a difference of two sums), in fp64 in the order of the norms with an exact 0 in place of a diagonal
 *    square.  Converged when off <= eps_T * fro and eps_T * fro is finite, both sides in fp64, eps_T = 2^-52 or 2^-23: a
 *    diagonal or zero matrix runs 0 sweeps.  Otherwise, after max_sweeps sweeps: stop, sweeps = -1.
 * 3. Round order.  A sweep is m - 1 rounds.  idx = [0 .. m-1]; a round pairs idx[k] with idx[m-1-k], k = 0 .. m/2 - 1; a pair
 *    that contains the padding index n (odd n) is dropped; p = min, q = max of the pair.  After a round
 *    idx = [idx[0], idx[m-1], idx[1], ..., idx[m-2]].  The list is reset at the start of every sweep (after m - 1 rounds it
 *    has returned to [0 .. m-1] by itself, so resetting and not resetting are the same order).
 * 4. Angles.  Of all pairs of a round from the matrix as it stands at the start of the round, with a_pq = a[p,q] (row p):
 *    tau = (a_qq - a_pp) / (a_pq + a_pq), t = copysign(1, tau) / (|tau| + sqrt(1 + tau*tau)), c = 1 / sqrt(1 + t*t), s = t * c.
 *    If a_pq == 0: c = 1, s = 0.  An overflowing tau or tau*tau gives t = 0 by itself; tau = 0 gives the 45 degree rotation.
 * 5. Apply.  Columns first, for all rows r: (a[r,p], a[r,q]) = (c*a[r,p] - s*a[r,q], s*a[r,p] + c*a[r,q]); V gets the same
 *    column update and nothing else.  Then, with every column of the round done, rows for all columns k:
 *    (a[p,k], a[q,k]) = (c*a[p,k] - s*a[q,k], s*a[p,k] + c*a[q,k]); then a[p,q] = a[q,p] = 0 exactly.  Rotations with c = 1,
 *    s = 0 are applied like any other.  The pairs of a round are disjoint: one writer per element and phase, no atomics.
 * 6. Finish.  The eigenvalues are the diagonal, ascending and stable: eigenvalue k goes to place
 *    #{j : d_j < d_k} + #{j < k : d_j == d_k}, and column k of V with it.
 * Non-finite input gives sweeps = -1 and unspecified values, and returns: the loop is bounded by max_sweeps.  An instance
 * computes the same bits alone or anywhere in any batch, with or without eigenvectors, with or without sweeps_dev.
 *
 * Errors follow dzo_pairwise_batch_hessian: unknown dtype, n < 1, batch outside 1 .. 2^30, a null matrices_dev or
 * eigenvalues_dev DZO_ERR_INVALID; n > DZO_SYMEIG_MAX_N DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required
 * DZO_ERR_ASSERT; no memory for the workspace DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_SYMEIG_MAX_N 384
#define DZO_SYMEIG_DEFAULT_SWEEPS 30
#define DZO_SYMEIG_STORAGE_LDS 0
#define DZO_SYMEIG_STORAGE_MEMORY 1
/* eigenvalues[b] (T, n per instance, ascending) and, unless eigenvectors_dev is NULL, eigenvectors[b] ((n, n), column-major,
 * column k belongs to eigenvalue k) of the symmetric part of matrices[b] ((n, n, batch), column-major per instance: the layout
 * dzo_pairwise_batch_hessian writes).  sweeps_dev (int32, batch) may be NULL: the sweeps instance b ran, or -1 when max_sweeps
 * were run without convergence.  max_sweeps <= 0: the default, 30.  matrices_dev is not modified.  Blocking. */
int32_t dzo_symmetric_batch_eigen(int64_t n, int64_t batch, int32_t dtype, const void *matrices_dev,
                                  void *eigenvalues_dev, void *eigenvectors_dev, int32_t *sweeps_dev, int32_t max_sweeps);
/* Where dzo_symmetric_batch_eigen keeps an n x n matrix of this dtype while it iterates: the storage, the leading dimension
 * and the dynamic LDS of the launch.  A pure function of (n, dtype): no device needed.  Any of the three outputs may be NULL.
 * Unknown dtype or n < 1 DZO_ERR_INVALID, n > DZO_SYMEIG_MAX_N DZO_ERR_UNSUPPORTED. */
int32_t dzo_symeig_plan(int64_t n, int32_t dtype, int32_t *storage, int64_t *ld, int64_t *lds_bytes);

/* ---------------------------------------------------------------------------------------
 * Batched eigenvector following (Cerjan-Miller / Wales) over many small Lennard-Jones clusters: the consumer of the two blocks
 * above.  Target index 0 is a Newton-quality minimiser: it polishes the points a quench leaves at is_stuck until the gradient
 * is at rounding level and the six rigid-body eigenvalues are zeros worth the name.  Target index 1 is a transition-state
 * search: every mode is stepped downhill but one followed mode, which is stepped uphill.  Nothing in the reference follows
 * modes: this block is the specification.  One 256-thread block per instance; 3N <= DZO_SYMEIG_MAX_N, so n_particles <=
 * DZO_MODEFOLLOW_MAX_PARTICLES = 128.
 *
 * Layout.  points, gradients, projections and follow vectors are (3N, batch): instance b at element 3N b, [x | y | z] -- the
 * layout of every cluster unit.  eigenvalues (3N, batch) and eigenvectors (3N, 3N, batch) are what dzo_symmetric_batch_eigen
 * writes.  Records are one value per instance: energies T; grms and step lengths fp64; status, index, zeros, followed mode,
 * sweeps int32; iteration counts int64.
 *
 * The step, per instance (T = the element type, n = 3N; every operation in T with one rounding, no contraction, IEEE division
 * and square root, unless fp64 is named).  Inputs: the point; lam[0..n) ascending and V (column i belongs to lam[i]), of the
 * Hessian AT THIS POINT; the followed vector w and whether it is set; target_index in {0, 1}, start_mode >= 0, max_step > 0,
 * zero_tol >= 0 (rounded once to T), grad_tol >= 0 (fp64).  An instance whose status is not ACTIVE is left alone.
 *  1. Evaluate.  E and g at the point, with the bits of dzo_pairwise_batch_energy_gradient (its routines and launch shapes).
 *  2. Gradient norm.  grms = sqrt((g.g)/n) in fp64: thread t = 0 .. 255 adds the squares of elements t, t + 256 by fused
 *     multiply-add from +0; the 64 values of a wave are added by the xor tree with offsets 32, 16, 8, 4, 2, 1; the four wave
 *     sums are added in wave order from +0 (the ORDER OF THE SUMS of this block; it depends on n only).
 *  3. Classify.  Mode i is a zero mode when |lam[i]| <= zero_tol; index = #{lam[i] < -zero_tol}; zeros = # of zero modes.
 *  4. Freeze check.  E, any g or any lam non-finite, or sweeps = -1 from the eigensolver: status FAILED.  Otherwise
 *     grms <= grad_tol (fp64): status CONVERGED.  In both cases the point is not moved, followed mode = -1, step length = 0,
 *     and the instance is frozen for all later steps with these records.
 *  5. Project.  F[i] = V[:,i].g in fp64: lane l = 0 .. 63 of a wave adds rows l, l + 64, ... by fused multiply-add from +0, then
 *     the xor tree; rounded once to T.
 *  6. Followed mode (target_index = 1 only).  w not set: the start_mode-th non-zero mode in ascending order (start_mode = 0 is
 *     the lowest); fewer non-zero modes than that: status FAILED, not moved.  w set: the non-zero mode with the largest
 *     |V[:,i].w| (the fp64 dot of step 5); ties go to the lowest i.  Then w = V[:,i*] as stored, sign included, and w is set.
 *  7. Mode steps.  a = |lam[i]|, q = (F[i] + F[i]) / a, h[i] = s * q / (1 + sqrt(1 + q*q)) with s = +1 for the followed mode
 *     and -1 for every other non-zero mode; h[i] = 0 for zero modes.  This is 2F / (a (1 + sqrt(1 + 4F^2/a^2))), bounded by 1
 *     in magnitude for any a.  An overflowing q*q gives h = 0 by itself.  (A q that itself overflows, 2|F| / a beyond the
 *     range of T, gives a NaN step: the next step's freeze check reports FAILED.  zero_tol > 0 keeps a away from that.)
 *  8. Cap.  hn = sqrt(sum h[i]^2) in fp64 in the order of the sums.  If hn > max_step (fp64), every h[i] is multiplied by
 *     T(max_step / hn), the quotient in fp64.
 *  9. Move.  x[r] = x[r] + d[r], d[r] = sum_i V[r,i] h[i] over i = 0 .. n-1 ascending from +0, one FUSED multiply-add per
 *     term (zero modes included: their terms add +-0).
 * 10. Record E, grms, index, zeros, the followed mode i* (-1 with target_index 0), the step length after the cap (max_step
 *     when the cap scaled the step, hn otherwise), status ACTIVE, iteration count += 1.  E, g and grms are those of the point
 *     BEFORE the move.
 * No floating-point atomics; one writer per element.  An instance computes the same bits alone or anywhere in any batch, and
 * a handle in one call of k steps or k calls of one.
 *
 * dzo_modefollow_batch_apply is the step, once, from modes the CALLER supplies (from anywhere: nothing in it depends on the
 * eigensolver); it sets every status to ACTIVE first.  Record outputs other than status_dev may be NULL; follow_dev and
 * follow_set_dev (int32, non-zero = set) may be NULL with target_index 0.  Blocking.
 * A handle ALIASES points_dev and owns Hessians, eigenvalues, eigenvectors, sweeps, follow vectors and the eigensolver's
 * workspace.  create leaves the energies and gradients of the points as given; the other records are zero until the first
 * step.  step enqueues, per step, dzo_pairwise_batch_hessian's launch, dzo_symmetric_batch_eigen's (with eigenvectors, default
 * sweeps) and the step kernel on the library's stream: no host wait between the three or between steps, one at the end for
 * all_done when it is not NULL.  Frozen instances still pass through the first two launches (same point, same bits).
 *
 * Errors follow dzo_pairwise_batch_hessian / dzo_symmetric_batch_eigen: unknown radial or dtype, sizes < 1, steps < 0, null
 * pointers, unknown `what`, target_index outside {0, 1}, start_mode < 0, max_step <= 0, a negative tolerance DZO_ERR_INVALID;
 * n_particles > 128 DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required DZO_ERR_ASSERT.
 * ------------------------------------------------------------------------------------- */
#define DZO_MODEFOLLOW_MAX_PARTICLES 128
/* status */
#define DZO_MODEFOLLOW_ACTIVE 0
#define DZO_MODEFOLLOW_CONVERGED 1
#define DZO_MODEFOLLOW_FAILED 2
/* `what` of get_ptr / read (T = the handle's element type) */
#define DZO_MODEFOLLOW_POINTS 0            /* T, 3N batch: the caller's array */
#define DZO_MODEFOLLOW_GRADIENTS 1         /* T, 3N batch: at the point before the last move */
#define DZO_MODEFOLLOW_ENERGIES 2          /* T, batch: likewise */
#define DZO_MODEFOLLOW_GRMS 3              /* fp64, batch */
#define DZO_MODEFOLLOW_STATUS 4            /* int32, batch */
#define DZO_MODEFOLLOW_INDEX 5             /* int32, batch: eigenvalues below -zero_tol */
#define DZO_MODEFOLLOW_ZEROS 6             /* int32, batch: eigenvalues within zero_tol of 0 */
#define DZO_MODEFOLLOW_FOLLOWED_MODE 7     /* int32, batch: i* of the last step, -1 when none */
#define DZO_MODEFOLLOW_STEP_LENGTHS 8      /* fp64, batch: of the last step, after the cap */
#define DZO_MODEFOLLOW_ITERATION_COUNTS 9  /* int64, batch: moves made */
#define DZO_MODEFOLLOW_EIGENVALUES 10      /* T, 3N batch: of the last step's Hessian */
#define DZO_MODEFOLLOW_EIGENVECTORS 11     /* T, (3N, 3N, batch) */
#define DZO_MODEFOLLOW_SWEEPS 12           /* int32, batch: the eigensolver's */
#define DZO_MODEFOLLOW_FOLLOW 13           /* T, 3N batch: the followed vectors w */
typedef struct dzo_modefollow_batch_s *dzo_modefollow_batch_t;
/* the step above, once, on every instance, from the caller's modes; points_dev is moved, follow_dev / follow_set_dev updated */
int32_t dzo_modefollow_batch_apply(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                   const void *eigenvalues_dev, const void *eigenvectors_dev, void *follow_dev,
                                   int32_t *follow_set_dev, int32_t target_index, int32_t start_mode, double max_step,
                                   double zero_tol, double grad_tol, void *energies_dev, void *gradients_dev,
                                   void *projections_dev, double *grms_dev, int32_t *status_dev, int32_t *index_dev,
                                   int32_t *zeros_dev, int32_t *followed_dev, double *step_lengths_dev);
/* points_dev: (3N, batch), ALIASED.  start_mode 0, no followed vector set.  Blocking. */
int32_t dzo_modefollow_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                    int32_t target_index, double max_step, double zero_tol, double grad_tol,
                                    dzo_modefollow_batch_t *out);
int32_t dzo_modefollow_batch_destroy(dzo_modefollow_batch_t h);
/* the mode an instance without a followed vector starts on (step 6) */
int32_t dzo_modefollow_batch_set_start_mode(dzo_modefollow_batch_t h, int32_t mode);
/* an initial followed vector w per instance: dirs_dev (3N, batch) is copied and every instance's w is set.  No wait. */
int32_t dzo_modefollow_batch_set_directions(dzo_modefollow_batch_t h, const void *dirs_dev);
/* `steps` steps of every ACTIVE instance; all_done may be NULL (then no host wait) */
int32_t dzo_modefollow_batch_step(dzo_modefollow_batch_t h, int32_t steps, int32_t *all_done);
/* instances with status ACTIVE.  Blocking. */
int32_t dzo_modefollow_batch_count_active(dzo_modefollow_batch_t h, int64_t *active);
/* device address of an array above (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_modefollow_batch_get_ptr(dzo_modefollow_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_modefollow_batch_read(dzo_modefollow_batch_t h, int32_t what, void *out_host);

/* ---------------------------------------------------------------------------------------
 * Batched lowest Hessian mode of many small Lennard-Jones clusters by restarted Lanczos inside ONE launch: "is this point a
 * minimum, and if not, which way is down?" for up to DZO_LOWMODE_MAX_PARTICLES = 1024 particles, from Hessian-vector products
 * alone -- the consumer of accelerated_pairwise_radial_hvp! (src/ExampleFunctions.jl:427-468).  No dense Hessian is formed.
 * Nothing in the reference iterates on that product: this block is the specification.  Stateless and blocking; each instance
 * runs at its own pace inside the launch.
 *
 * Layout.  points, start and vectors are (3N, batch): instance b at element 3N b, [x | y | z] -- the layout of every cluster
 * unit.  eigenvalues are T, (batch); residuals fp64, (batch), may be NULL; info is int32, (3, batch), may be NULL: status at
 * 3 b, cycles at 3 b + 1, products at 3 b + 2.  start_dev may be NULL: the start is then drawn in the kernel.
 *
 * Launch shapes.  n_particles <= 64: one wave per instance, lane i holds particle i and its entries of the current vector in
 * registers, the Lanczos basis (3 * 64 * K elements) lives in dynamic LDS.  65 .. 1024: one 256-thread block per instance,
 * thread t owns particles t + 256 q, point and current vector staged in LDS, the basis in a per-call device workspace of
 * 3N * K * batch elements (a thread reads back only what it wrote itself), freed before the call returns.
 *
 * Arithmetic (T = the element type; n = 3N; every operation rounded once, no contraction, IEEE division and square root;
 * "fp64" names the operations done in double precision on values converted exactly from T).
 *  a. Sums.  Every sum over the particles is in fp64 in THE ORDER OF THE SUMS, which depends on N only: N <= 64: lane i holds
 *     the term of particle i (+0 beyond N), added by the xor tree with offsets 32, 16, 8, 4, 2, 1.  Above: thread t adds the
 *     terms of particles t, t + 256, ... in that order from +0 (+0 for a particle beyond N), the 64 values of a wave are
 *     added by the same tree, the four wave sums are added in wave order from +0.  (For N <= 64 the single wave sum is added
 *     to +0 likewise.)  A dot a.b has the term a_x b_x, then fma(a_y, b_y, .), then fma(a_z, b_z, .) per particle, as in
 *     dzo_pairwise_batch_hvp.
 *  b. Product.  H v is dzo_pairwise_batch_hvp's products of the point with the direction v: the same pair term, the same row
 *     loop, the same order, hence the same bits.
 *  c. Projector (project_rigid != 0; otherwise P is the identity and steps c and d are skipped).  Once per instance, all fp64,
 *     plain products and sums: centroid c_a = (sum_i r_a,i) / N; rho_i = r_i - c; the unit-mass inertia tensor
 *     Gxx = sum(rho_y rho_y + rho_z rho_z), Gyy = sum(rho_x rho_x + rho_z rho_z), Gzz = sum(rho_x rho_x + rho_y rho_y),
 *     Gxy = -sum(rho_x rho_y), Gxz = -sum(rho_x rho_z), Gyz = -sum(rho_y rho_z).  Cofactors A00 = Gyy Gzz - Gyz Gyz,
 *     A01 = Gxz Gyz - Gxy Gzz, A02 = Gxy Gyz - Gxz Gyy, A11 = Gxx Gzz - Gxz Gxz, A12 = Gxy Gxz - Gxx Gyz,
 *     A22 = Gxx Gyy - Gxy Gxy; det = Gxx A00 + Gxy A01 + Gxz A02 (left to right); tr = Gxx + Gyy + Gzz.  The instance is
 *     FAILED (cycles = products = 0, eigenvalue and residual NaN) unless det > 2^-36 (tr tr) tr, a test that a singular G
 *     (collinear particles: det is rounding noise, some 2^-50 tr^3) and a non-finite one both fail.  Otherwise I_ab = A_ab / det.
 *  d. P v (result in T): m_a = (sum_i v_a,i) / N; L = sum_i rho_i x v_i, per particle Lx: rho_y v_z - rho_z v_y, Ly:
 *     rho_z v_x - rho_x v_z, Lz: rho_x v_y - rho_y v_x (two products and a difference); omega_a = I_ax Lx + I_ay Ly + I_az Lz
 *     (left to right); (P v)_x,i = T((v_x,i - m_x) - (omega_y rho_z,i - omega_z rho_y,i)), y: omega_z rho_x - omega_x rho_z,
 *     z: omega_x rho_y - omega_y rho_x.
 *  e. normalise(v): s = sqrt(v.v) (fp64), r = 1 / s, v_e = T(v_e r).  The operator is A v = P (H v) on vectors that are
 *     themselves P of something: A = P H P up to the rounding of the projection.
 *  f. Start.  u = start[b], or drawn: particle i takes draws 4 i .. 4 i + 3 of the PCG32 stream whose state after seeding is
 *     advance(0x14057B7EF767814F + base_seed + b) (the rule of basin hopping) as d1 .. d4 of the tempering rule: three
 *     normals (x, y, z) by Box-Muller in fp64, each rounded to T.  u = P u, then normalise; s zero or non-finite: FAILED.
 *  g. A cycle on the unit vector u = q_0, with K = min(krylov, dimension of the range of P) (n - 6 with project_rigid, n
 *     without), for j = 0 .. K - 1:
 *       w = A q_j (products += 1); h_k = q_k.w for k = 0 .. j, all from this w (CLASSICAL Gram-Schmidt); alpha_j = h_j.
 *       j = K - 1 > 0: the cycle ends here.
 *       w_e = T(((w_e - h_0 q_0,e) - h_1 q_1,e) - ...), fp64, one product and one difference per k.
 *       j = 0: alpha_1 = alpha_0, beta_1 = sqrt(w.w): the Rayleigh quotient of u and the norm of w - alpha_1 u, its residual.
 *         scale = max(scale, |alpha_1|) (scale starts at 0; a NaN never enters).  beta_1 <= res_tol scale: CONVERGED with
 *         eigenvalue T(alpha_1), vector u, residual beta_1.  Otherwise, in cycle max_cycles: UNFINISHED with the same three.
 *       A second pass: h_k = q_k.w, w updated as above.  beta_j = sqrt(w.w); unless beta_j > 0 the cycle ends with j + 1 steps
 *       (an exact zero or a NaN).  w_e = T(w_e (1 / beta_j)).
 *       Clean-up, at most four passes: w = P w; h_k = q_k.w and the update as above; s = sqrt(w.w); unless s > 0 the cycle
 *       ends with j + 1 steps; w_e = T(w_e (1 / s)); a pass with s > 0.7 is the last.  (Once the Krylov space has closed, w is
 *       amplified rounding noise and carries rigid-body components: without this pass the 13-atom icosahedron never
 *       converges.)  q_(j+1) = w.
 *  h. Ritz pair of the k x k tridiagonal (k = the steps of the cycle; diagonal alpha_0 .. alpha_(k-1), off-diagonal
 *     beta_0 .. beta_(k-2)) in fp64: cyclic Jacobi by the round order, angles and apply rules of dzo_symmetric_batch_eigen's
 *     items 3-5 with T = double and V = I at the start.  At the start of every sweep: off_c = the sum over rows r != c
 *     ascending of a[r,c]^2 from +0, dia_c = a[c,c]^2; off2 and dia2 are their sums over c by the xor tree of 64 lanes (+0
 *     beyond k); the iteration ends when off2 <= 2^-104 (off2 + dia2), or after 30 sweeps.  theta = the smallest diagonal
 *     entry (the lowest index among equals), y its column of V.  scale = max(scale, |theta|).
 *     u_e = T(((0 + y_0 q_0,e) + y_1 q_1,e) + ...) in fp64; u = P u; normalise; s zero or non-finite: FAILED.  Next cycle.
 * No floating-point atomics, every output element is written once.  Nothing loops without a bound: at most max_cycles K
 * products.  An instance computes the same bits alone or anywhere in any batch for a given start vector, drawn or supplied.
 *
 * Errors are those of dzo_pairwise_batch_hessian: unknown radial or dtype, sizes < 1, a null points_dev, eigenvalues_dev or
 * vectors_dev DZO_ERR_INVALID; n_particles > 1024 DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required
 * DZO_ERR_ASSERT.  krylov outside 2 .. DZO_LOWMODE_MAX_KRYLOV, max_cycles < 1, a negative or non-finite res_tol, project_rigid
 * with n_particles < 3 DZO_ERR_INVALID; no memory for the workspace DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_LOWMODE_MAX_PARTICLES 1024
#define DZO_LOWMODE_MAX_KRYLOV 32
/* status */
#define DZO_LOWMODE_CONVERGED 0
#define DZO_LOWMODE_UNFINISHED 1
#define DZO_LOWMODE_FAILED 2
/* the lowest eigenpair of P H P (project_rigid != 0: net translation and rotation removed) or of H at every points[b] */
int32_t dzo_pairwise_batch_lowest_mode(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype,
                                       const void *points_dev, int32_t project_rigid, int32_t krylov, int32_t max_cycles,
                                       double res_tol, uint64_t base_seed, const void *start_dev, void *eigenvalues_dev,
                                       void *vectors_dev, double *residuals_dev, int32_t *info_dev);

/* ---------------------------------------------------------------------------------------
 * Batched hybrid eigenvector following (Munro & Wales 1999) over many Lennard-Jones clusters: a transition-state search
 * that never forms a Hessian, the consumer of the start_dev argument of the block above.  Per step the lowest mode is refined
 * from the previous step's vector by a few Hessian-vector products; the point then steps uphill along that mode and relaxes
 * in the subspace orthogonal to it by a few gradient evaluations.  Up to DZO_HYBRIDEF_MAX_PARTICLES = 1024 particles, where
 * the dense search stops at 128.  Nothing in the reference follows modes: this block is the specification.
 *
 * Layout.  points, gradients and modes are (3N, batch): instance b at element 3N b, [x | y | z] -- the layout of every
 * cluster unit.  Records are one value per instance: energies, eigenvalues, projections F and uphill steps h in T; grms and
 * mode residuals fp64; status and tangent steps int32; iteration counts, products and evaluations int64.
 *
 * Launch shapes of the step kernel.  n_particles <= 64: one wave per instance, lane i holds particle i.  65 .. 1024: one
 * 256-thread block per instance, thread t owns particles t + 256 q.  Point, mode, gradient and the previous tangent point and
 * projected gradient live in registers.
 *
 * The step, per instance (T = the element type, n = 3N; every operation in T with one rounding, no contraction, IEEE division
 * and square root, unless fp64 is named; "fp64" names operations in double precision on values converted exactly from T).
 * Every sum over the particles is in fp64 in THE ORDER OF THE SUMS of the block above (its item a), a dot a.b with its three
 * terms per particle.  Inputs: the point x; a unit vector u and a value lam, the lowest mode of the Hessian AT THIS POINT
 * with net translation and rotation projected out, and that mode's status; max_step > 0, tangent_cap > 0, tangent_first > 0,
 * grad_tol >= 0 (all fp64), zero_tol >= 0 (rounded once to T), tangent_steps >= 0, tangent_steps_convex >= 0.  An instance
 * whose status is not ACTIVE is left alone.
 *  1. Evaluate.  E and g at x, with the bits of dzo_pairwise_batch_energy_gradient (its routines and launch shapes).
 *     grms = sqrt((g.g)/n) in fp64.
 *  2. Freeze check.  E, g.g (which any non-finite g makes non-finite) or lam non-finite, or the mode's status FAILED: status
 *     FAILED.  Otherwise grms <= grad_tol (fp64): status CONVERGED.  In both cases the point is not moved, F = h = 0,
 *     tangent steps = 0, and the instance is frozen for all later steps with these records.
 *  3. Uphill step.  F = T(u.g), the dot in fp64.  a = |lam|.  If a <= zero_tol, h = 0; otherwise q = (F + F) / a and
 *     h = q / (1 + sqrt(1 + q*q)) -- 2F / (a (1 + sqrt(1 + 4F^2/a^2))), bounded by 1 in magnitude -- which is invariant to
 *     the sign of u: F and h change sign with it, h u does not.  If |h| > max_step (compared in fp64), h = +-T(max_step).
 *     x_e = fma(h, u_e, x_e), one FUSED multiply-add per element.
 *  4. Tangent relaxation: tangent_steps iterations when lam < -zero_tol, otherwise tangent_steps_convex (a search still
 *     inside the basin of its minimum is not to be pulled back).  For t = 0, 1, ...: g' = the gradient at x as in item 1;
 *     c = u.g' (fp64); p_e = T(g'_e - c u_e), the product and the difference in fp64; pp = p.p (fp64).  If
 *     sqrt(pp / n) <= grad_tol the loop ends.  alpha = tangent_first at t = 0; for t > 0, with s = x - x_prev and
 *     y = p - p_prev (both in T), alpha = (s.s) / (s.y) in fp64 if s.y > 0, else tangent_first: the Barzilai-Borwein
 *     length.  dn = alpha sqrt(pp) (fp64); if dn > tangent_cap, alpha = alpha (tangent_cap / dn) in fp64.  x_prev = x,
 *     p_prev = p, x_e = fma(-T(alpha), p_e, x_e).
 *  5. Record, all of the point BEFORE the move: E, g and grms; lam, u and the mode's residual; F and h; the tangent
 *     iterations that moved the point; products += the mode's products and evaluations += 1 + the gradients of item 4
 *     (both cumulative; a step that freezes counts what it spent); status ACTIVE; iteration count += 1.
 * No floating-point atomics; one writer per element; nothing loops without a bound.  An instance computes the same bits alone
 * or anywhere in any batch, and a handle in one call of k steps or k calls of one.
 * CONVERGED says only that the point is stationary: lam tells whether it is a saddle (lam < -zero_tol), and only the full
 * spectrum tells its index.  The method can end on a saddle of higher index; that is known behaviour, not an error.
 *
 * dzo_hybridef_batch_apply is the step, once, from a mode (u, lam) the CALLER supplies (from anywhere: nothing in it depends
 * on the Lanczos iteration); it sets every status to ACTIVE first.  Record outputs other than status_dev may be NULL.  Blocking.
 * A handle ALIASES points_dev and owns the modes of record u, a second mode buffer, the records and, above 64 particles, the
 * Lanczos workspace of 3N * krylov * batch elements.  create copies dirs_dev (3N, batch) into u, or, with dirs_dev NULL, lets
 * the first refinement draw its start in the kernel from base_seed (item f of the block above); it leaves the energies and
 * gradients of the points as given, the other records zero until the first step.  step enqueues, per step, two launches on
 * the library's stream: dzo_pairwise_batch_lowest_mode's kernel with project_rigid = 1, K = krylov, res_tol = mode_tol and
 * start = u, writing into the second buffer; then the step kernel, which reads the mode from there and, for the instances it
 * found ACTIVE, copies it into u (so a frozen instance keeps its mode of record to the bit).  The mode launch runs
 * mode_cycles + 1 cycles at most: a cycle of that iteration ends with the Ritz vector, and the first product of the next
 * measures its eigenvalue and residual, so mode_cycles cycles of krylov products refine and one product measures; a mode
 * whose residual passes mode_tol at the first product costs that one product.  Its status UNFINISHED is normal here; only
 * FAILED matters.  No host wait between the two launches or between steps, one at the end for all_done when it is not NULL.
 * Frozen instances still pass through the mode launch.
 *
 * Errors follow dzo_pairwise_batch_lowest_mode: unknown radial or dtype, batch < 1, n_particles < 3 (rigid projection
 * needs 3 particles), steps < 0, null pointers, unknown `what`, max_step, tangent_cap or tangent_first <= 0, a negative
 * count or tolerance, krylov outside 2 .. DZO_LOWMODE_MAX_KRYLOV, mode_cycles < 1, a non-finite mode_tol DZO_ERR_INVALID;
 * n_particles > 1024 DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required DZO_ERR_ASSERT; no memory for
 * the state DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_HYBRIDEF_MAX_PARTICLES 1024
/* status */
#define DZO_HYBRIDEF_ACTIVE 0
#define DZO_HYBRIDEF_CONVERGED 1
#define DZO_HYBRIDEF_FAILED 2
/* `what` of get_ptr / read (T = the handle's element type) */
#define DZO_HYBRIDEF_POINTS 0              /* T, 3N batch: the caller's array */
#define DZO_HYBRIDEF_GRADIENTS 1           /* T, 3N batch: at the point before the last move */
#define DZO_HYBRIDEF_ENERGIES 2            /* T, batch: likewise */
#define DZO_HYBRIDEF_GRMS 3                /* fp64, batch */
#define DZO_HYBRIDEF_STATUS 4              /* int32, batch */
#define DZO_HYBRIDEF_EIGENVALUES 5         /* T, batch: lam of the last step */
#define DZO_HYBRIDEF_MODES 6               /* T, 3N batch: u of the last step */
#define DZO_HYBRIDEF_MODE_RESIDUALS 7      /* fp64, batch: of the mode launch of the last step */
#define DZO_HYBRIDEF_PROJECTIONS 8         /* T, batch: F */
#define DZO_HYBRIDEF_UPHILL_STEPS 9        /* T, batch: h after the cap */
#define DZO_HYBRIDEF_TANGENT_STEPS 10      /* int32, batch: tangent iterations of the last step that moved the point */
#define DZO_HYBRIDEF_ITERATION_COUNTS 11   /* int64, batch: moves made */
#define DZO_HYBRIDEF_PRODUCTS 12           /* int64, batch: Hessian-vector products, cumulative */
#define DZO_HYBRIDEF_EVALUATIONS 13        /* int64, batch: gradient evaluations, cumulative */
typedef struct dzo_hybridef_batch_s *dzo_hybridef_batch_t;
/* the step above, once, on every instance, from the caller's modes; points_dev is moved */
int32_t dzo_hybridef_batch_apply(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                 const void *eigenvalues_dev, const void *modes_dev, double max_step, int32_t tangent_steps,
                                 int32_t tangent_steps_convex, double tangent_cap, double tangent_first, double zero_tol,
                                 double grad_tol, void *energies_dev, void *gradients_dev, void *projections_dev,
                                 void *uphill_steps_dev, double *grms_dev, int32_t *status_dev, int32_t *tangent_counts_dev);
/* points_dev: (3N, batch), ALIASED.  dirs_dev: (3N, batch) first modes, copied, or NULL.  Blocking. */
int32_t dzo_hybridef_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                  const void *dirs_dev, double max_step, int32_t tangent_steps, int32_t tangent_steps_convex,
                                  double tangent_cap, double tangent_first, int32_t krylov, int32_t mode_cycles,
                                  double mode_tol, double zero_tol, double grad_tol, uint64_t base_seed,
                                  dzo_hybridef_batch_t *out);
int32_t dzo_hybridef_batch_destroy(dzo_hybridef_batch_t h);
/* the mode the next refinement of every instance starts from: dirs_dev (3N, batch) is copied into u.  No wait. */
int32_t dzo_hybridef_batch_set_directions(dzo_hybridef_batch_t h, const void *dirs_dev);
/* `steps` steps of every ACTIVE instance; all_done may be NULL (then no host wait) */
int32_t dzo_hybridef_batch_step(dzo_hybridef_batch_t h, int32_t steps, int32_t *all_done);
/* instances with status ACTIVE.  Blocking. */
int32_t dzo_hybridef_batch_count_active(dzo_hybridef_batch_t h, int64_t *active);
/* device address of an array above (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_hybridef_batch_get_ptr(dzo_hybridef_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_hybridef_batch_read(dzo_hybridef_batch_t h, int32_t what, void *out_host);

/* ---------------------------------------------------------------------------------------
 * Structure fingerprints and their classification: which of many Lennard-Jones clusters are the same structure up to
 * rotation, translation, reflection and a relabelling of the particles.  Every unit above ends in a (3N, batch) array of
 * stationary points most of which are copies of each other; these two entries say how many distinct ones there are and which.
 *
 * dzo_structure_batch_fingerprint, one launch for the whole batch, up to DZO_STRUCTURE_MAX_PARTICLES = 1024 particles (one
 * wave per instance up to 64 particles, one 256-thread block above; the point and then the sort buffers in 24 KiB of LDS at
 * most, so there is no device-memory fallback).  T is the element type.  Per instance:
 *   1. e_i = sum_{j != i} e(r2_ij), summed in T from +0 with j ascending, the pair term that of the pairwise objective with the
 *      self term dropped by a select: the bits of the row sums behind dzo_pairwise_batch_energy_gradient.
 *   2. E = (T)(0.5 * sum_i e_i), the rows added in fp64 in THE ORDER OF THE SUMS of the block above (a thread's particles in
 *      order, the wave tree, the four waves in wave order): E has the bits of dzo_pairwise_batch_energy_gradient.  Written to
 *      energies_dev unless that is NULL.
 *   3. c = (sum_i r_i) / N per coordinate: the sum in fp64 in the same order, one division in fp64, one rounding to T.
 *      d_i = (x_i - c_x)^2 + (y_i - c_y)^2 + (z_i - c_z)^2 in T, the squares added left to right.
 *   4. fingerprint = [e sorted ascending (N) | d sorted ascending (N)], instance b at 2N b.  The sort is an exact in-kernel
 *      bitonic sort of the values, padded with +inf to a power of two.  Values that are not numbers sort last, behind +inf, and
 *      are written as the canonical quiet NaN; -0 sorts before +0.
 * No floating-point atomics; every output element is written once; an instance computes the same bits alone or anywhere in
 * any batch.  The call enqueues and then blocks.
 * What the fingerprint does NOT do: it does not tell a structure from its mirror image, and two different structures could
 * in principle share it.  It is the identification GMIN-style programs use (energy plus sorted invariants), made stricter by
 * the per-particle energies.  A coincident pair of particles gives a fingerprint with elements that are not finite.
 * Errors: unknown radial or dtype, n_particles < 1, batch outside 1 .. 2^30, null points or fingerprints DZO_ERR_INVALID;
 * n_particles > 1024 DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required DZO_ERR_ASSERT.
 *
 * dzo_structure_batch_classify labels `batch` vectors of `length` elements (instance b at length b; fingerprints, or
 * fingerprints with descriptors of the caller's appended: length is free).  The match rule, evaluated in fp64: a and b match
 * iff for every i  |a_i - b_i| <= tol * max(1, |a_i|, |b_i|).  An instance with any non-finite element matches nothing and
 * gets label -1.  Labels are greedy leader labels in index order: instance k takes the label of the first REPRESENTATIVE
 * j < k it matches; if there is none, k becomes a representative with label k.  *n_classes is the number of representatives.
 * This is deliberately not "the smallest matching index": matching is not transitive (a ~ b, b ~ c, a !~ c gives 0, 0, 2),
 * and a label always names a representative.  Known structures placed first in the batch make the call "match against a
 * database": as long as they are distinct from each other they keep their own labels.
 * One launch fills the lower triangle of a batch x batch bit matrix (a pair's comparison leaves at the first failing element),
 * one single-wave launch walks k = 0 .. batch-1 over its rows masked by the representatives so far.  The result does not
 * depend on grid size or scheduling.  The matrix, batch^2 / 8 bytes (32 MiB at DZO_STRUCTURE_MAX_BATCH = 16384), is allocated
 * and freed by the call.  The call blocks: it returns *n_classes (host memory).
 * Errors: tol < 0 or not a number, length < 1, batch < 1, unknown dtype, null pointers DZO_ERR_INVALID; batch > 16384
 * DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required DZO_ERR_ASSERT; no memory for the matrix DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_STRUCTURE_MAX_PARTICLES 1024
#define DZO_STRUCTURE_MAX_BATCH 16384
int32_t dzo_structure_batch_fingerprint(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype,
                                        const void *points_dev,    /* T, (3N, batch), the quench layout [x|y|z] */
                                        void *fingerprints_dev,    /* T, (2N, batch) */
                                        void *energies_dev);       /* T, batch; may be NULL */
int32_t dzo_structure_batch_classify(int64_t length, int64_t batch, int32_t dtype, const void *fingerprints_dev, /* T, (length, batch) */
                                     double tol, int32_t *labels_dev /* int32, batch */, int32_t *n_classes /* host */);

/* ---------------------------------------------------------------------------------------
 * Batched nudged elastic band with a climbing image (Henkelman & Jonsson 2000; Henkelman, Uberuaga & Jonsson 2000) over many
 * pairs of Lennard-Jones minima: the double-ended search.  The mode-following units above start from one point and end where
 * they end; a band is strung between two GIVEN minima and relaxed until its highest image sits on the saddle that joins them.
 * Its output is what those units consume: a transition-state candidate (the climbing image) with a direction (its tangent).
 * Nothing in the reference relaxes a band: this block is the specification.
 *
 * Layout.  A band is n_images = M images of an N-particle cluster; image m of band b sits at element 3N (M b + m), [x | y | z]:
 * the whole array is a (3N, M batch) points array that dzo_pairwise_batch_energy_gradient evaluates as it is.  Images 0 and
 * M-1 are the fixed ends.  velocities, forces and tangents have the band's layout (zero at the ends); energies and force_rms
 * are M per band; residuals, climbing and highest image, status and iteration count are one per band.
 * 3 <= n_images <= DZO_NEB_MAX_IMAGES = 32, n_particles <= DZO_NEB_MAX_PARTICLES = 1024.  The ends must be given in a common
 * frame (no rigid or permutational alignment is done here; the two quenched sides of one saddle are in one).
 *
 * Launch shapes of the step kernel (dzo_neb_plan tells).  One 256-thread block per band, `steps` iterations per launch, the
 * phases of an iteration separated by workgroup barriers only: no grid-wide synchronisation, no atomics, no host wait inside or
 * between launches.  DZO_NEB_SHAPE_WAVE, n_particles <= 64: the interior images are dealt round-robin to the four waves
 * (image m to wave (m - 1) mod 4), lane i holds particle i.  DZO_NEB_SHAPE_BLOCK, 65 .. 1024: the block takes the images one
 * after another, thread t owns particles t + 256 q, the image under evaluation staged in LDS.  DZO_NEB_STORAGE_LDS: band,
 * velocities and forces live in LDS for the whole launch, whenever 768 bytes, the stage (3N elements, BLOCK shape only) and
 * 3 * 3N M elements fit the 159 KiB of dynamic LDS the cluster units allow; that always holds for the WAVE shape.  Otherwise
 * DZO_NEB_STORAGE_MEMORY: the same kernel body on the caller's band and the handle's velocities and forces in device memory.
 * Both storages compute the same bits.
 *
 * One iteration, per band (T = the element type, n = 3N; every operation in T with one rounding, no contraction, IEEE division
 * and square root, unless fp64 is named; "fp64" names operations in double precision on values converted exactly from T).
 * Every sum over the particles is in fp64 in THE ORDER OF THE SUMS of the cluster units (a thread's particles in order, the wave
 * tree, in the BLOCK shape the four waves in wave order), a dot a.b with its three terms per particle.  Inputs: the band x, the
 * velocities v; spring > 0, dt > 0, max_move > 0, force_tol >= 0 (all fp64; dt also rounded once to T), climb, climb_after.
 * A band whose status is not ACTIVE is left alone.
 *  1. Evaluate.  E_m and g_m of every interior image, with the bits of dzo_pairwise_batch_energy_gradient.  The ends are
 *     evaluated once, at create (by apply: in the call), and feel no force.
 *  2. Improved tangent of every interior m.  d+ = x_{m+1} - x_m and d- = x_m - x_{m-1}, element by element in T.
 *     If E_{m+1} > E_m > E_{m-1}: t = d+.  If E_{m+1} < E_m < E_{m-1}: t = d-.  Otherwise, with (in T)
 *     a = max(|E_{m+1} - E_m|, |E_{m-1} - E_m|) and b = min of the same two: t_e = fma(a, d+_e, b d-_e) if E_{m+1} > E_{m-1},
 *     else t_e = fma(b, d+_e, a d-_e).  tau_e = T(t_e / sqrt(t.t)), the root and the quotient in fp64: unit length.
 *  3. Force.  c = g_m.tau (fp64), w = spring (sqrt(d+.d+) - sqrt(d-.d-)) (fp64).
 *     F_e = T(-(g_e - c tau_e) + w tau_e), every operation in fp64: the gradient with its component along the band taken
 *     out, and the spring force along the band only.  The climbing image feels F_e = T(-g_e + (c + c) tau_e) instead: the
 *     gradient with its component along the band turned uphill, no spring.  The climbing image exists when climb != 0 and the
 *     band's iteration count is >= climb_after (apply: when climb != 0); it is the interior image of highest E, the first one
 *     in index order (compared with > in T).
 *  4. Residual and status.  frms_m = sqrt((F_m.F_m) / n) in fp64, residual = max_m frms_m.  Any E_m (the ends included) or
 *     F_m.F_m non-finite (which any non-finite g or F makes so): status FAILED.  Otherwise residual <= force_tol: status
 *     CONVERGED.  In both cases nothing moves, and the band is frozen for all later iterations with these records.
 *  5. Move, per interior image, by projected velocity Verlet.  p = v.F (fp64).  If p > 0, v_e = T((p / F.F) F_e), quotient
 *     and product in fp64; else v_e = 0.  v_e = fma(T(dt), F_e, v_e).  s_e = T(dt) v_e.  If sqrt(s.s) > max_move (fp64),
 *     s_e = T((max_move / sqrt(s.s)) s_e) in fp64.  x_e = x_e + s_e.  Iteration count += 1.
 *  6. Every force of an iteration is computed from the band as it stood at the start of that iteration, not from images
 *     already moved.
 * The records are those of the band BEFORE the move of the last iteration made: energies, forces, tangents, force_rms (zero
 * at the ends), residual, the climbing image (-1 while none climbs) and the highest image.
 * No floating-point atomics; one writer per element; every loop is bounded by an argument.  A band computes the same bits alone
 * or anywhere in any batch, and a handle in one call of k steps or k calls of one.
 * CONVERGED says that the forces of the band vanish to force_tol.  With a climbing image that makes the climbing image a
 * stationary point of the energy to force_tol; whether it is a first-order saddle is for the spectrum to say.
 * Out of scope: alignment of arbitrary end pairs, the doubly-nudged spring term, L-BFGS on the band, other radials.
 *
 * dzo_neb_batch_interpolate writes the straight band between a_dev and b_dev (3N, batch): images 0 and M-1 are copies of a
 * and b, and x_m = fma(T(m / (M-1)), b - a, a) in between (the quotient in fp64, rounded once).  One launch; blocking.
 * dzo_neb_batch_apply is ONE iteration from the caller's band and velocities (both moved); it sets every status to ACTIVE
 * first and evaluates the ends itself.  Record outputs other than status_dev may be NULL; gradients_dev receives g of every
 * image, the ends included.  Blocking.
 * A handle ALIASES band_dev and owns the velocities (zero at create) and the records; create evaluates the ends.  step
 * enqueues ONE launch for `steps` iterations; all_done may be NULL (then no host wait).
 *
 * Errors follow the neighbours: unknown radial or dtype, sizes < 1, n_images outside 3 .. 32, spring, dt or max_move <= 0, a
 * negative tolerance or count, null pointers, unknown `what` DZO_ERR_INVALID; n_particles > 1024 DZO_ERR_UNSUPPORTED; a host
 * pointer where a device pointer is required DZO_ERR_ASSERT; no memory for the state DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_NEB_MAX_PARTICLES 1024
#define DZO_NEB_MAX_IMAGES 32
/* status */
#define DZO_NEB_ACTIVE 0
#define DZO_NEB_CONVERGED 1
#define DZO_NEB_FAILED 2
/* what dzo_neb_plan tells */
#define DZO_NEB_SHAPE_WAVE 0
#define DZO_NEB_SHAPE_BLOCK 1
#define DZO_NEB_STORAGE_LDS 0
#define DZO_NEB_STORAGE_MEMORY 1
/* `what` of get_ptr / read (T = the handle's element type, M = n_images) */
#define DZO_NEB_BAND 0                /* T, 3N M batch: the caller's array */
#define DZO_NEB_VELOCITIES 1          /* T, 3N M batch */
#define DZO_NEB_FORCES 2              /* T, 3N M batch: F of the last iteration, before its move */
#define DZO_NEB_TANGENTS 3            /* T, 3N M batch: tau likewise */
#define DZO_NEB_ENERGIES 4            /* T, M batch */
#define DZO_NEB_FORCE_RMS 5           /* fp64, M batch */
#define DZO_NEB_RESIDUALS 6           /* fp64, batch */
#define DZO_NEB_CLIMBING_IMAGES 7     /* int32, batch: -1 before climbing starts */
#define DZO_NEB_HIGHEST_IMAGES 8      /* int32, batch */
#define DZO_NEB_STATUS 9              /* int32, batch */
#define DZO_NEB_ITERATION_COUNTS 10   /* int64, batch: moves made */
typedef struct dzo_neb_batch_s *dzo_neb_batch_t;
/* launch shape, storage and dynamic LDS of a band; a pure function, needs no device.  Outputs may be NULL. */
int32_t dzo_neb_plan(int64_t n_particles, int32_t n_images, int32_t dtype, int32_t *shape, int32_t *storage, int64_t *lds_bytes);
/* a_dev, b_dev: (3N, batch).  band_dev: (3N, M batch), written. */
int32_t dzo_neb_batch_interpolate(int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, const void *a_dev,
                                  const void *b_dev, void *band_dev);
/* the iteration above, once, on every band, from the caller's band and velocities */
int32_t dzo_neb_batch_apply(int32_t radial, int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, void *band_dev,
                            void *velocities_dev, double spring, double dt, double max_move, double force_tol, int32_t climb,
                            void *energies_dev, void *gradients_dev, void *forces_dev, void *tangents_dev,
                            double *force_rms_dev, double *residuals_dev, int32_t *climbing_dev, int32_t *highest_dev,
                            int32_t *status_dev);
/* band_dev: (3N, M batch), ALIASED.  Blocking. */
int32_t dzo_neb_batch_create(int32_t radial, int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, void *band_dev,
                             double spring, double dt, double max_move, double force_tol, int32_t climb, int64_t climb_after,
                             dzo_neb_batch_t *out);
int32_t dzo_neb_batch_destroy(dzo_neb_batch_t h);
/* `steps` iterations of every ACTIVE band in one launch; all_done may be NULL (then no host wait) */
int32_t dzo_neb_batch_step(dzo_neb_batch_t h, int32_t steps, int32_t *all_done);
/* bands with status ACTIVE.  Blocking. */
int32_t dzo_neb_batch_count_active(dzo_neb_batch_t h, int64_t *active);
/* device address of an array above (no wait) / a blocking copy of it to host memory, in the array's own element type */
int32_t dzo_neb_batch_get_ptr(dzo_neb_batch_t h, int32_t what, void **ptr_dev);
int32_t dzo_neb_batch_read(dzo_neb_batch_t h, int32_t what, void *out_host);

/* ---------------------------------------------------------------------------------------
 * Batched rigid and permutational alignment of pairs of clusters of identical particles (the minpermdist of Wales' OPTIM, as
 * used in GMIN / PATHSAMPLE): for every pair (A, B) a rotation R, a sign s and a permutation p that make
 * sum_i |a_i - R s b_p(i)|^2 small, centroids removed.  dzo_neb_batch_* and the double-ended search built on it need their two
 * ends in a common frame and leave "alignment of arbitrary end pairs" out of scope: this block supplies it.  Nothing in the
 * reference aligns structures: this block is the specification.  No potential is involved, so there is no `radial`.
 *
 * a_dev and b_dev are (3N, batch), pair k [x | y | z] at element 3N k, the layout of every dzo_*_batch_* unit; neither is
 * changed.  1 <= n_particles <= DZO_ALIGN_MAX_PARTICLES = 1024.  All arithmetic below is fp64 on values widened exactly from T,
 * every operation rounded once, no contraction except the fma named, IEEE division and square root; so the permutations do
 * not depend on the element type beyond the input values.
 *
 * THE ORDER OF EVERY SUM over particles: column j (a particle of B) belongs to lane j mod 64 of the pair's wave; a lane adds
 * the terms of its columns j = l, l + 64, ... in that order onto 0, lanes without a column hold 0, and the 64 lane sums are
 * added by the wave tree of the dzo_*_batch_* units (offsets 32, 16, 8, 4, 2, 1).  A sum over rows i is taken over the columns
 * j = p(i) in this order.
 *
 * Assignment (dzo_align_batch_assign, and step 1 of a cycle): the permutation p, row i of A -> column p(i) of B, that
 * minimises sum_i c(i, p(i)), c(i, j) = fma(dz, dz, fma(dy, dy, dx dx)) with dx = a_i.x - b_j.x and dy, dz alike.  No N x N
 * matrix is stored.  The method is the shortest augmenting path with row potentials u and column potentials v, all zero at
 * the start.  Rows are taken in index order.  For row i: every slack is +inf, no column is visited; the path starts at a
 * virtual column whose row is i.  Repeat, at most N + 1 times: let i0 be the row of the path's last column; for every
 * unvisited column j ascending, cur = (c(i0, j) - u[i0]) - v[j], and if cur < slack[j] then slack[j] = cur and the
 * predecessor of j is the path's last column; delta = the smallest slack of the unvisited columns, j1 the lowest column that
 * has it; u += delta on the rows of the visited columns and on row i, v -= delta on the visited columns, slack -= delta on
 * the unvisited ones; j1 is visited and becomes the path's last column; stop when j1 has no row.  Then the rows move one
 * column along the predecessors, from j1 back to the virtual column.  cost_dev = sum_i c(i, p(i)) in the order above.
 *
 * Pairs (dzo_align_batch_pairs).  c_A and c_B are the centroids (the sum of each coordinate, divided by N); a_i and b_j below
 * are a_i - c_A and s (b_j - c_B).  Starts: n_orient first rotations R_0, in this order: the identity, if trials has
 * DZO_ALIGN_TRIAL_IDENTITY; the four principal ones, if it has DZO_ALIGN_TRIAL_PRINCIPAL; random_trials random ones
 * (<= DZO_ALIGN_MAX_RANDOM_TRIALS = 64).  With allow_inversion the same n_orient rotations follow once more with s = -1:
 * n_starts = (allow_inversion ? 2 : 1) n_orient, start t has orientation t mod n_orient.
 *   Principal: the second moments (xx, xy, xz, yy, yz, zz; sums of plain products) of A and of B make two symmetric 3 x 3
 *   matrices; cyclic Jacobi (below) gives their eigenvectors; the columns are ordered by eigenvalue ascending, equal ones by
 *   index, and the third is negated if the determinant is negative: frames F_A, F_B.  R_0 = F_A D F_B^T, element (r, c) =
 *   (d0 F_A[r][0] F_B[c][0] + d1 F_A[r][1] F_B[c][1]) + d2 F_A[r][2] F_B[c][2], D = (+,+,+), (+,-,-), (-,+,-), (-,-,+).
 *   Random: the PCG32 XSH-RR stream of dzo_tempering_* seeded with `seed` (state = A (C + seed) + C), jumped ahead by
 *   4 r draws for random trial r.  Every pair of a call is given the same random rotations: the stream is selected by the seed
 *   and the trial index alone, so a pair draws the same numbers alone or anywhere in a batch, and with any other trial
 *   count.  The draws d1 .. d4 give u_m = (d_m + 1/2) 2^-32, r1 = sqrt(-2 log u1), r2 = sqrt(-2 log u3), the
 *   quaternion (w, x, y, z) = (r1 cospi(2 u2), r1 sinpi(2 u2), r2 cospi(2 u4), r2 sinpi(2 u4)), four standard normals, and
 *   R_0 is its rotation (below).  The inverted copy of a random start uses the same rotation.
 * One cycle of a start, at most max_cycles (<= DZO_ALIGN_MAX_CYCLES = 64): (1) b'_j = R b_j, each coordinate
 * (R0 x + R1 y) + R2 z, and the assignment above between A and b'; (2) Horn's rotation for that assignment: the nine sums
 * S_uv = sum b_p(i).u a_i.v, the symmetric 4 x 4 matrix H00 = (Sxx + Syy) + Szz, H11 = (Sxx - Syy) - Szz,
 * H22 = (Syy - Sxx) - Szz, H33 = (Szz - Sxx) - Syy, H01 = Syz - Szy, H02 = Szx - Sxz, H03 = Sxy - Syx, H12 = Sxy + Syx,
 * H13 = Szx + Sxz, H23 = Syz + Szy, its eigenvectors by cyclic Jacobi, the one of the largest eigenvalue (the first among
 * equals) as the quaternion (w, x, y, z); R is its rotation.  The start ends DZO_ALIGN_CONVERGED when a cycle's permutation
 * is the previous cycle's (so after two cycles at least), DZO_ALIGN_CYCLE_LIMIT after max_cycles cycles.  Its distance is
 * sqrt(sum_i |a_i - R b_p(i)|^2) with the last permutation and the last rotation, the squares as in c(i, j).
 *   Rotation of a quaternion: n = sqrt((ww + xx) + (yy + zz)), every component divided by n, then R00 = (ww + xx) - (yy + zz),
 *   R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = (ww - xx) + (yy - zz), R12 = 2 (yz - wx),
 *   R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = (ww - xx) - (yy - zz).
 *   Cyclic Jacobi of a D x D matrix M: V = 1; at most 12 sweeps over the pairs (p, q), p < q, in row order; a pair with
 *   M_pq == 0 is skipped, a sweep that skips every pair ends it.  theta = (M_qq - M_pp) / (M_pq + M_pq),
 *   g = sqrt(theta theta + 1), t = 1 / (theta + g) if theta >= 0 else -1 / (g - theta), c = 1 / sqrt(t t + 1), s = t c; for
 *   every k columns p and q of M and of V become (c m_kp - s m_kq, s m_kp + c m_kq), then rows p and q of M likewise, then
 *   M_pq = M_qp = 0.  Eigenvalues are the diagonal, eigenvectors the columns of V.  N = 1 and N = 2 give rank-deficient
 *   matrices and finite answers: a zero matrix keeps V = 1.
 * The pair's result is the start with the smallest distance, the first in index order among equals; status_dev, cycles_dev
 * and best_trial_dev are that start's.  aligned_dev: x'_i = ((R0 x + R1 y) + R2 z) + c_A.x ... of (b_p(i) - c_B) with the
 * signed rotation s R, rounded once to T: B in A's frame with A's labels, so dzo_neb_batch_interpolate(a, aligned) is the
 * straight band.  perm_dev: p, int32 (N, batch).  rotation_dev: s R, row-major, fp64 (9, batch), det = +-1.  distance_dev:
 * from the unrounded values.  trial_distances_dev: every start's distance, (n_starts, batch); may be NULL.
 * A pair with any non-finite coordinate is detected before any loop runs: status DZO_ALIGN_FAILED, the identity permutation,
 * aligned = b, the identity rotation, distance (every trial distance; the cost of assign) NaN, cycles and best trial 0.
 *
 * Launches: one wave per (pair, start), batch n_starts independent waves; lane l holds the rotated coordinates, potentials,
 * slacks and visited flags of columns l + 64 q in registers (instantiated for 1, 4 and 16 columns per lane: N <= 64, 256,
 * 1024); A, the row potentials and three 16-bit index arrays in LDS, 38 N + 8 bytes: 38 920 at N = 1024, four waves per
 * compute unit of 160 KiB, one per SIMD.  The argmin is a wave reduction through DPP and permlane moves: a column scan waits
 * for no other wave.  A second kernel, one wave per pair, picks the best start and writes the outputs.  No floating-point
 * atomics, no atomics at all; every output element is written once; every loop is bounded by a count known at entry (a path
 * by N + 1 columns, the cycles by max_cycles, a Jacobi by its 12 sweeps) and no NaN can keep one alive: the next column is an
 * index out of the unvisited ones whatever the values are.  A pair computes the same bits alone or anywhere in any batch.
 * Both calls block; the workspace (192 + 4 N bytes per start) is allocated and freed inside the call.
 * Out of scope: several atom species (every particle may take every place), point-group symmetry detection, and a guarantee
 * of the global minimum: the method is a multi-start local one, and its distance is an upper bound of the true one.
 *
 * Errors follow the neighbours: sizes < 1, unknown dtype, unknown bits in trials, negative counts, max_cycles < 1, null required
 * pointers, trials == 0 && random_trials == 0 DZO_ERR_INVALID; n_particles, random_trials or max_cycles above its limit
 * DZO_ERR_UNSUPPORTED; a host pointer where a device pointer is required DZO_ERR_ASSERT; no memory for the workspace
 * DZO_ERR_NOMEM.
 * ------------------------------------------------------------------------------------- */
#define DZO_ALIGN_MAX_PARTICLES 1024
#define DZO_ALIGN_MAX_RANDOM_TRIALS 64
#define DZO_ALIGN_MAX_CYCLES 64
/* bits of `trials` */
#define DZO_ALIGN_TRIAL_IDENTITY 1
#define DZO_ALIGN_TRIAL_PRINCIPAL 2
/* status */
#define DZO_ALIGN_CONVERGED 0
#define DZO_ALIGN_CYCLE_LIMIT 1
#define DZO_ALIGN_FAILED 2
int32_t dzo_align_batch_assign(int64_t n_particles, int64_t batch, int32_t dtype, const void *a_dev, const void *b_dev, /* T, (3N, batch) */
                               int32_t *perm_dev /* int32, (N, batch) */, double *cost_dev /* fp64, batch */);
int32_t dzo_align_batch_pairs(int64_t n_particles, int64_t batch, int32_t dtype, const void *a_dev, const void *b_dev, /* T, (3N, batch) */
                              int32_t trials /* DZO_ALIGN_TRIAL_* bits */, int32_t random_trials, int32_t max_cycles,
                              int32_t allow_inversion, uint64_t seed, void *aligned_dev /* T, (3N, batch) */,
                              int32_t *perm_dev /* int32, (N, batch) */, double *rotation_dev /* fp64, (9, batch) */,
                              double *distance_dev /* fp64, batch */, int32_t *best_trial_dev, int32_t *cycles_dev,
                              int32_t *status_dev /* int32, batch each */,
                              double *trial_distances_dev /* fp64, (n_starts, batch); may be NULL */);

/* ---------------------------------------------------------------------------------------
 * Transition-state candidates of many bands (the candidate step of the connect cycle of Carr, Trygubenko & Wales 2005, the
 * method of Wales' OPTIM): a band between two minima that are several elementary steps apart does not converge, and does not
 * have to.  Every local maximum of its energy profile is a candidate for a transition state, with the band's tangent there as
 * the first mode of a refinement (dzo_hybridef_batch_*).  dzo_pathway_batch_candidates takes the candidates of `batch` bands
 * and compacts them.  Nothing in the reference does this: this block is the specification.  No potential is evaluated (the
 * caller supplies the energies), so there is no `radial`.
 *
 * band_dev is (3N, M batch), the layout of dzo_neb_batch_*: image m of band b sits at element 3N (M b + m), [x | y | z].
 * energies_dev is (M, batch) in T, for instance DZO_NEB_ENERGIES of a handle or dzo_pairwise_batch_energy_gradient of the band
 * taken as M batch points.  Neither is changed.  1 <= n_particles <= DZO_PATHWAY_MAX_PARTICLES = 1024,
 * 3 <= n_images <= DZO_PATHWAY_MAX_IMAGES = 32, 1 <= batch <= DZO_PATHWAY_MAX_BATCH = 1048576.
 *
 * Candidate rule.  Interior image m, 1 <= m <= M-2, of band b is a candidate iff E_m > E_{m-1} and E_m >= E_{m+1}, plain
 * comparisons in T.  So a plateau E_m == E_{m+1} yields its first image only, E_m == E_{m-1} is no candidate, a NaN on either
 * side of a comparison yields nothing, and the ends are never candidates.  A band holds at most (M - 1) / 2 candidates.
 * Order.  Candidates are numbered band-major, the image index ascending inside a band: offsets_dev[b] is the number of
 * candidates of the bands before b, offsets_dev[batch] the count; candidate offsets_dev[b] + k is the k-th of band b.
 * Per candidate c (band b, image m): points_dev row c = x_m, copied; candidate_energies_dev[c] = E_m, copied;
 * band_index_dev[c] = b, image_index_dev[c] = m; tangents_dev row c = tau, the improved tangent of the band rule of
 * dzo_neb_batch_* (its item 2), restated: d+ = x_{m+1} - x_m and d- = x_m - x_{m-1}, element by element in T.
 * If E_{m+1} > E_m > E_{m-1}: t = d+.  If E_{m+1} < E_m < E_{m-1}: t = d-.  Otherwise, with (in T)
 * a = max(|E_{m+1} - E_m|, |E_{m-1} - E_m|) and b = min of the same two: t_e = fma(a, d+_e, b d-_e) if E_{m+1} > E_{m-1}, else
 * t_e = fma(b, d+_e, a d-_e).  (A candidate always takes the third case.)  tau_e = T(t_e / sqrt(t.t)), the root and the quotient
 * in fp64.  t.t is in fp64 in the order of the sums of dzo_neb_batch_* for the same N: three terms per particle (a product and
 * two fused multiply-adds), a thread's particles in order, the wave tree, and for N > 64 the four waves in wave order.  So a
 * candidate's tangent is bit for bit the tangent dzo_neb_batch_apply records for image m of the same band, and t.t == 0 (two
 * neighbours on top of the image) gives the same NaN row.
 *
 * Capacity.  The five candidate arrays hold `capacity` rows.  If the count exceeds it, candidates capacity, capacity + 1, ...
 * are not written, offsets_dev and *count are complete all the same, and the call returns DZO_PATHWAY_OVERFLOW = 7 (not a
 * failure of the device: call again with room for *count).  With capacity == 0 the five arrays may be NULL: the call counts.
 *
 * Launches: three on one stream and one host wait at the end, for the count.  (1) One thread per band counts its candidates from
 * its energies.  (2) ONE 256-thread block turns the counts into exclusive offsets in place: thread t adds the counts of bands
 * t per .. (t + 1) per - 1, per = ceil(batch / 256), the 256 run sums are scanned in LDS, and the thread writes its run's
 * offsets; integers, so no order matters, and any batch up to the bound is one pass.  (3) One 256-thread block per band reads
 * the band's energies into LDS, finds the candidates again and writes its slice: for N <= 64 candidate k goes to wave k mod 4
 * and lane i holds particle i, for 65 <= N <= 1024 the block takes the candidates in turn and thread t owns particles
 * t, t + 256, ...  No read-modify-write on memory, one writer per element, every loop is bounded by an argument; a band computes
 * the same bits alone or anywhere in any batch.  The call blocks.
 * Out of scope: evaluating the band (dzo_pairwise_batch_energy_gradient does), the refinement, and the cycle that owns the
 * database of minima and saddles (the host modules' connect_pathways).
 *
 * Errors follow the neighbours: unknown dtype, sizes < 1, n_images outside 3 .. 32, a negative capacity, null pointers
 * DZO_ERR_INVALID; n_particles > 1024 or batch > DZO_PATHWAY_MAX_BATCH DZO_ERR_UNSUPPORTED; a host pointer where a device
 * pointer is required DZO_ERR_ASSERT.
 * ------------------------------------------------------------------------------------- */
#define DZO_PATHWAY_MAX_PARTICLES 1024
#define DZO_PATHWAY_MAX_IMAGES 32
#define DZO_PATHWAY_MAX_BATCH 1048576
/* returned when the count exceeds the capacity */
#define DZO_PATHWAY_OVERFLOW 7
int32_t dzo_pathway_batch_candidates(int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype,
                                     const void *band_dev /* T, (3N, M batch) */, const void *energies_dev /* T, (M, batch) */,
                                     int64_t capacity, void *points_dev, void *tangents_dev /* T, (3N, capacity) each */,
                                     void *candidate_energies_dev /* T, capacity */, int32_t *band_index_dev,
                                     int32_t *image_index_dev /* int32, capacity each */, int32_t *offsets_dev /* int32, batch + 1 */,
                                     int64_t *count /* host */);

/* ---------------------------------------------------------------------------------------
 * LBFGSOptimizer  (src/DZOptimization.jl:321-509)
 * ------------------------------------------------------------------------------------- */
/* Full constructor (:347-397).  ALIASES x_dev and g_dev as current_point / current_gradient
 * exactly as the reference aliases initial_point / initial_gradient (:393,:395); allocates
 * delta_point, delta_gradient (zero-filled), step_direction = -step*g/|g| and the (s, y)
 * ring.  initial_step_length <= 0 -> DZO_ERR_ASSERT (:380).  history_length must be 1..64. */
int32_t dzo_lbfgs_create(int64_t n, int32_t history_length, int32_t dtype, void *x_dev,
                         void *g_dev, double initial_objective_value,
                         double initial_step_length, dzo_lbfgs_t *out);
/* Convenience constructor (:400-427): checks the constraint, evaluates f0 and g0 through the
 * callbacks into a library-owned gradient vector, then calls the full constructor. */
int32_t dzo_lbfgs_create_callbacks(dzo_constraint_fn constraint, dzo_objective_fn objective,
                                   dzo_gradient_fn gradient, void *ctx, int64_t n,
                                   int32_t history_length, int32_t dtype, void *x_dev,
                                   double initial_step_length, dzo_lbfgs_t *out);
/* Same with a built-in problem as the callback triple (constraint = nothing). */
int32_t dzo_lbfgs_create_problem(dzo_problem_t problem, int32_t history_length, void *x_dev,
                                 double initial_step_length, dzo_lbfgs_t *out);
int32_t dzo_lbfgs_destroy(dzo_lbfgs_t opt);
int32_t dzo_lbfgs_set_callbacks(dzo_lbfgs_t opt, dzo_constraint_fn constraint,
                                dzo_objective_fn objective, dzo_gradient_fn gradient, void *ctx);
int32_t dzo_lbfgs_set_problem(dzo_lbfgs_t opt, dzo_problem_t problem);
int32_t dzo_lbfgs_set_two_loop_mode(dzo_lbfgs_t opt, int32_t mode);
int32_t dzo_lbfgs_set_max_halvings(dzo_lbfgs_t opt, int64_t max_halvings);

/* Optional safeguards, OFF by default (off = the live reference's step!).  SURVEY.md 8(f):
 *   descent_check  -- legacy/DZOptimization.jl:682-692: after the two-loop, if g.d is not
 *       finite the optimizer stops (is_stuck); if g.d >= 0 the direction is replaced by
 *       -(last_step_length/||g||) g, last_step_length = ||delta_point|| of the last step (:625-627).
 *   steepest_descent_fallback -- legacy :588-610: when the search along a quasi-Newton direction
 *       fails, retry along -(last_step_length/||g||) g; success clears the (s, y) history
 *       (_history_count[] = 0, :609), failure sets is_stuck.
 * dzo_lbfgs_get_i fields 8 / 9 / 10: history resets, descent-check replacements, kind of the
 * last step (0 quasi-Newton, 1 replaced by the descent check, 2 fallback); fields 11 / 12: steps
 * taken as one sweep over the history (single-pass step) and how many of those had their first
 * trial rejected; field 13: how many of the rejected ones were continued by the same pass at
 * t/2; field 14: layout of the history in HBM -- 0 slabs, 1 tiles of pairs, 2 tiles of points
 * (DESIGN.md "point ring"); field 15: arrangement of the tiles -- 1 tile-major, 2 stream-major
 * (informational); field 16: 1 when the pass over the point ring recomputes the points' gradients from the
 * point tiles instead of streaming them; field 17: register sets per wave of that pass (1 = two waves per
 * SIMD, 2 = one), 0 when the optimizer is not on the point ring (both informational); field 18: steps that first
 * compared the aliased arrays with the point ring because a pointer to them had been handed out (dzo_lbfgs_read hands
 * out none);
 * dzo_lbfgs_get_s field 2: last_step_length. */
int32_t dzo_lbfgs_set_safeguards(dzo_lbfgs_t opt, int32_t descent_check, int32_t steepest_descent_fallback);

/* Line search used by step!: DZO_LINE_SEARCH_BACKTRACKING (reference, default) or
 * DZO_LINE_SEARCH_WOLFE -- the consumer of the quotients the reference's LineSearchEvaluator
 * defines but never uses (src/DZOptimization.jl:84 improvement_ratio, :88-89 slope_ratio):
 * bisection / doubling from t = 1 until improvement_ratio >= c1 and |slope_ratio| <= c2, at most
 * max_evals evaluator calls (each = objective + gradient at the trial point).  Guarantees
 * delta_point . delta_gradient > 0 for every pushed pair.  The accepted trial gradient becomes
 * current_gradient (no extra gradient call).  c1, c2, max_evals <= 0 keep the defaults
 * (1e-4, 0.9, 40). */
int32_t dzo_lbfgs_set_line_search(dzo_lbfgs_t opt, int32_t kind, double c1, double c2, int32_t max_evals);

/* step!(opt) (:454-509) -- the whole step, callbacks invoked from inside. */
int32_t dzo_lbfgs_step(dzo_lbfgs_t opt);

/* Split entry points for hosts that drive the loop themselves (the objective / gradient
 * callbacks run between them, :138 and :479):
 *   direction      compute_lbfgs_step_direction! (:430-451), K1
 *   begin_search   copy!(delta_point, current_point) (:118)
 *   trial          axpy!(t, d, x) from the saved point + isequal test (:124,:128), K2
 *   accept         delta_f, f, delta_point = x - x_old (:142-145), K3
 *   reject         copy!(x, delta_point) (:151), K4
 *   pre_gradient   copy!(delta_gradient, g) (:478)
 *   post_gradient  delta_gradient = g - delta_gradient, ring push, rho, count (:480-507), K5+K6
 * dzo_lbfgs_direction only enqueues its kernels on the optimizer's stream (like a KernelAbstractions
 * launch); dzo_lbfgs_get_ptr(4) or dzo_synchronize waits for step_direction. */
int32_t dzo_lbfgs_direction(dzo_lbfgs_t opt);
int32_t dzo_lbfgs_begin_search(dzo_lbfgs_t opt);
int32_t dzo_lbfgs_trial(dzo_lbfgs_t opt, double step_size, int32_t *changed);
int32_t dzo_lbfgs_accept(dzo_lbfgs_t opt, double next_objective_value);
int32_t dzo_lbfgs_reject(dzo_lbfgs_t opt);
int32_t dzo_lbfgs_pre_gradient(dzo_lbfgs_t opt);
int32_t dzo_lbfgs_post_gradient(dzo_lbfgs_t opt);

/* State (all of it is public in the reference, README.md:11).
 * get_i:   0 is_stuck  1 iteration_count  2 n  3 history_length  4 length(history)
 *          5 objective evaluations in the last step  6 two-loop mode  7 dtype
 * get_s:   0 current_objective_value  1 delta_objective_value
 * get_ptr: 0 current_point  1 delta_point  2 current_gradient  3 delta_gradient
 *          4 step_direction  5 delta_point_history[idx]  6 delta_gradient_history[idx]
 *          (idx 0 = newest, the reference's index 1)
 * Validity: 0 and 2 are the arrays the constructor was given (aliased, :393) and stay valid for the
 * optimizer's life; a get_ptr / dzo_synchronize / dzo_memcpy_* call settles the live copy into them.
 * 1, 3 and 4 are valid until the next step.  An optimizer made by dzo_lbfgs_create_problem on the
 * built-in chained Rosenbrock with history_length <= 20 keeps its history tile-major in HBM (DESIGN.md,
 * "blocked ring" / "point ring"): for it 1, 3, 4, 5 and 6 return contiguous COPIES formed by the call, valid
 * until the next step -- read-only; install pairs with dzo_lbfgs_set_history.  Every other optimizer
 * returns the live vectors. */
int32_t dzo_lbfgs_get_i(dzo_lbfgs_t opt, int32_t what, int64_t *value);
int32_t dzo_lbfgs_get_s(dzo_lbfgs_t opt, int32_t what, double *value);
int32_t dzo_lbfgs_set_s(dzo_lbfgs_t opt, int32_t what, double value);
int32_t dzo_lbfgs_set_stuck(dzo_lbfgs_t opt, int32_t is_stuck);
int32_t dzo_lbfgs_get_ptr(dzo_lbfgs_t opt, int32_t what, int32_t idx, void **ptr_dev);
/* Field `what` (get_ptr's numbering; n elements of the optimizer's dtype) copied to host memory, synchronously.  Unlike
 * get_ptr this hands out no pointer: the host cannot have written into current_point / current_gradient through it, so the
 * step behind a read does not have to check the aliased arrays against the optimizer's own state (after get_ptr,
 * dzo_synchronize or dzo_memcpy_* it does: the reference's step! walks from whatever those arrays hold, :393).  The way to
 * watch an optimization from the host. */
int32_t dzo_lbfgs_read(dzo_lbfgs_t opt, int32_t what, int32_t idx, void *host_dst);
/* rho_history / alpha_history (:341-342), newest first; *count receives the length */
int32_t dzo_lbfgs_get_rho(dzo_lbfgs_t opt, double *out, int32_t capacity, int32_t *count);
int32_t dzo_lbfgs_get_alpha(dzo_lbfgs_t opt, double *out, int32_t capacity, int32_t *count);
/* Install k pairs (rows of S_dev / Y_dev, k x n row-major, row 0 newest) and, optionally,
 * their rho = s.y values; used for checkpoint/resume and frozen-state parity tests. */
int32_t dzo_lbfgs_set_history(dzo_lbfgs_t opt, int32_t k, const void *S_dev, const void *Y_dev,
                              const double *rho_or_null, int64_t iteration_count);
int32_t dzo_lbfgs_stream(dzo_lbfgs_t opt, void **hip_stream);

/* ---------------------------------------------------------------------------------------
 * LineSearchEvaluator call (src/DZOptimization.jl:65-92): trial point x + t*d, objective,
 * Armijo quotient (:84) and, optionally, trial gradient + curvature quotient (:85-90).
 * ------------------------------------------------------------------------------------- */
int32_t dzo_line_search_eval(dzo_constraint_fn constraint, dzo_objective_fn objective,
                             dzo_gradient_fn gradient, void *ctx, int64_t n, int32_t dtype,
                             const void *x_dev, double current_objective_value,
                             const void *d_dev, double overlap, double step_size,
                             int32_t compute_gradient, void *trial_point_dev,
                             void *trial_gradient_dev, double *trial_objective_value,
                             double *improvement_ratio, double *slope_ratio);

/* ---------------------------------------------------------------------------------------
 * AdGDOptimizer (src/DZOptimization.jl:179-312) -- SURVEY.md 8(f) rank 1
 * ------------------------------------------------------------------------------------- */
int32_t dzo_adgd_create(int64_t n, int32_t dtype, void *x_dev, void *g_dev,
                        double initial_objective_value, double initial_step_length,
                        dzo_adgd_t *out);
int32_t dzo_adgd_create_problem(dzo_problem_t problem, void *x_dev, double initial_step_length,
                                dzo_adgd_t *out);
int32_t dzo_adgd_destroy(dzo_adgd_t opt);
int32_t dzo_adgd_set_callbacks(dzo_adgd_t opt, dzo_constraint_fn constraint,
                               dzo_objective_fn objective, dzo_gradient_fn gradient, void *ctx);
int32_t dzo_adgd_step(dzo_adgd_t opt);
/* With the built-in chained Rosenbrock objective step! is ONE pass over x and g (first trial, objective,
 * gradient, both deltas and the two norms the next step's :292-294 need) that reads x and g and writes
 * the trial point and its gradient into twin buffers (6 n T of traffic); after a rejected trial the pass
 * is repeated at half the step from the untouched x and g (:151-152).
 * get_i: 0 is_stuck 1 iteration_count 2 n 3 fused steps 4 of them after a rejected first trial
 *        5 passes that were already in flight when their step! was called (the next pass is enqueued behind
 *        every decision, its step size from the device-side evaluation of :285-299 / :152)
 *        6 passes in flight that were dropped (a pointer was handed out, an option changed)
 *        7 adopted passes whose device-side step size differed from the host's evaluation (expected 0)
 *        8 steps that took the generic kernels because the caller's current_gradient array (which the optimizer
 *          aliases, src/DZOptimization.jl:216-239, and step! walks along, :301) no longer held the gradient of the
 *          current point when the step began -- the host wrote into it, or passed its own initial_gradient;
 * get_s: 0 f 1 delta_f 2 current_step_size 3 previous_step_size;
 * get_ptr: 0 x 1 delta_point 2 g 3 delta_gradient.  0 and 2 are the constructor's arrays (aliased, :261)
 * for the optimizer's life: get_ptr / dzo_synchronize / dzo_memcpy_* settle the live copy into them.
 * 1 and 3 are valid until the next step (delta_gradient alternates between two buffers). */
int32_t dzo_adgd_get_i(dzo_adgd_t opt, int32_t what, int64_t *value);
int32_t dzo_adgd_get_s(dzo_adgd_t opt, int32_t what, double *value);
int32_t dzo_adgd_get_ptr(dzo_adgd_t opt, int32_t what, void **ptr_dev);
/* as dzo_lbfgs_read: field `what` to host memory without handing out a pointer */
int32_t dzo_adgd_read(dzo_adgd_t opt, int32_t what, void *host_dst);

/* ---------------------------------------------------------------------------------------
 * BFGSOptimizer (legacy/DZOptimization.jl:733-994; README.md:33-41)
 * ------------------------------------------------------------------------------------- */
/* Constructor (:762-810): COPIES x0 (:769), evaluates f0 / g0, H0 = I (:783), d0 = g (:784),
 * last_step_length = initial_step_length (:779).  Argument order objective, gradient,
 * constraint follows :762-766.  constraint may be NULL (NULL_CONSTRAINT, :759). */
int32_t dzo_bfgs_create_callbacks(dzo_objective_fn objective, dzo_gradient_fn gradient,
                                  dzo_constraint_fn constraint, void *ctx, int64_t n,
                                  int32_t dtype, const void *x0_dev, double initial_step_length,
                                  dzo_bfgs_t *out);
int32_t dzo_bfgs_create_problem(dzo_problem_t problem, const void *x0_dev,
                                double initial_step_length, dzo_bfgs_t *out);
/* Re-precision constructors BFGSOptimizer(::Type{T}, opt) / (::Type{T}, f, g!, c!, opt)
 * (legacy/DZOptimization.jl:812-862): a NEW optimizer of the target element type that continues
 * from `src`: x, H, delta_point, delta_gradient are converted elementwise (T.(..)), f and g are
 * re-evaluated in the new precision, d = H*g is recomputed (:833-836), iteration_count /
 * last_step_length / last_step_type carry over, has_terminated restarts as false (:849).
 * The target type is the new problem's dtype, or `dtype` for the callback form. */
int32_t dzo_bfgs_convert_problem(dzo_bfgs_t src, dzo_problem_t problem_of_target_dtype, dzo_bfgs_t *out);
int32_t dzo_bfgs_convert_callbacks(dzo_bfgs_t src, int32_t dtype, dzo_objective_fn objective,
                                   dzo_gradient_fn gradient, dzo_constraint_fn constraint, void *ctx,
                                   dzo_bfgs_t *out);
int32_t dzo_bfgs_destroy(dzo_bfgs_t opt);
/* step!(opt) (:891-994): competitive quadratic line searches, accept / reset / terminate. */
int32_t dzo_bfgs_step(dzo_bfgs_t opt);
/* update_inverse_hessian! (:864-889) on raw device arrays: rescales d in place (:874),
 * t = H*dg into scratch (:875), rank-2 update of H (:878-886).  If g_dev and d_next_dev are
 * non-NULL the next direction d_next = H_new*g (:958-960) is produced in the same pass. */
int32_t dzo_bfgs_update(int64_t n, int32_t dtype, void *H_dev, double step_length, void *d_dev,
                        const void *dg_dev, void *scratch_dev, const void *g_dev,
                        void *d_next_dev);
/* The same update with the rank-2 term on the matrix cores (v_mfma_f64_16x16x4_f64, K = 2 padded
 * to 4): fp64, n % 16 == 0, H only (no fused direction).  A measured alternative, NOT the default:
 * the kernel is HBM-bound either way, rounding follows an fma chain instead of :882-884 and H loses
 * bit-exact symmetry. */
int32_t dzo_bfgs_update_mfma(int64_t n, int32_t dtype, void *H_dev, double step_length, void *d_dev,
                             const void *dg_dev, void *scratch_dev);
/* out = H*v for symmetric H (mul!, :875,:958-960) */
int32_t dzo_symv(int64_t n, int32_t dtype, const void *H_dev, const void *v_dev, void *out_dev);
/* quadratic_line_search(functor, f0, t0) as defined in DESIGN.md from
 * find_three_point_bracket (:49-172) + QuadraticLineSearch (:191-216); direction 0 = -g, 1 = -d */
int32_t dzo_bfgs_line_search(dzo_bfgs_t opt, int32_t use_gradient_direction, double t0,
                             double *t_best, double *f_best);
int32_t dzo_bfgs_set_max_increases(dzo_bfgs_t opt, int32_t max_increases);
/* approximate_inverse_hessian <- I (identity_matrix!, :712-720) and next_step_direction <- gradient:
 * the reset step! performs itself after a gradient-descent step (:981-986), for hosts that restart. */
int32_t dzo_bfgs_reset(dzo_bfgs_t opt);
/* get_i: 0 has_terminated (== has_converged, README.md:38) 1 iteration_count 2 n
 *        3 last_step_type 4 objective evaluations so far
 * get_s: 0 current_objective_value 1 last_step_length
 * get_ptr: 0 current_point 1 delta_point 2 current_gradient 3 delta_gradient
 *          4 next_step_direction 5 approximate_inverse_hessian 6 scratch */
int32_t dzo_bfgs_get_i(dzo_bfgs_t opt, int32_t what, int64_t *value);
int32_t dzo_bfgs_get_s(dzo_bfgs_t opt, int32_t what, double *value);
int32_t dzo_bfgs_get_ptr(dzo_bfgs_t opt, int32_t what, void **ptr_dev);
/* Install state ("save/load data in the middle of optimization", README.md:11; the re-precision
 * constructor :812-862 moves a whole optimizer the same way).  The device arrays (x, g, delta_point,
 * delta_gradient, next_step_direction, H) are the optimizer's state itself: write them through the
 * pointers of dzo_bfgs_get_ptr (dzo_memcpy_h2d / d2d) between steps.  The host-side fields:
 *   set_s: 0 current_objective_value (NaN -> DZO_ERR_ASSERT, :773)  1 last_step_length
 *          2 delta_objective_value (gradient-descent handles)
 *   set_i: 0 has_terminated  1 iteration_count  3 last_step_type  4 objective evaluations so far */
int32_t dzo_bfgs_set_s(dzo_bfgs_t opt, int32_t what, double value);
int32_t dzo_bfgs_set_i(dzo_bfgs_t opt, int32_t what, int64_t value);

/* ---------------------------------------------------------------------------------------
 * Legacy GradientDescentOptimizer (legacy/DZOptimization.jl:305-449) with
 * QuadraticLineSearch() (:181-216) as its line_search_function!.  Argument order constraint,
 * objective, gradient follows :330-337.  The handle type and the getters are the BFGS ones
 * (dzo_bfgs_get_i / get_s / get_ptr / destroy; get_s field 2 = delta_objective_value, get_ptr
 * field 4 = next_step_direction = -last_step_length * g/|g|, field 5 is NULL: no Hessian).
 * ------------------------------------------------------------------------------------- */
int32_t dzo_gd_create_callbacks(dzo_constraint_fn constraint, dzo_objective_fn objective,
                                dzo_gradient_fn gradient, void *ctx, int64_t n, int32_t dtype,
                                const void *x0_dev, double initial_step_length, dzo_bfgs_t *out);
int32_t dzo_gd_create_problem(dzo_problem_t problem, const void *x0_dev, double initial_step_length,
                              dzo_bfgs_t *out);
/* step!(opt) (:393-449) */
int32_t dzo_gd_step(dzo_bfgs_t opt);

/* ---------------------------------------------------------------------------------------
 * Batched dense BFGS: B independent BFGSOptimizer instances on one device, one workgroup per
 * instance, the whole step (both line searches included) on the device.  "run multiple
 * optimizers in parallel" (README.md:12); instances shard over the GPUs of a node with no data-path
 * collective, only the convergence flag is all-reduced (dzo_comm_* below).  The step kernel keeps
 * the LOWER triangle of every inverse Hessian only (H is symmetric bit for bit); dzo_bfgs_batch_get_ptr
 * mirrors it before handing out H.
 * ------------------------------------------------------------------------------------- */
int32_t dzo_bfgs_batch_create(int32_t problem_kind, int64_t batch, int64_t n, int32_t dtype,
                              const void *x0_dev /* batch x n row-major */,
                              double initial_step_length, dzo_bfgs_batch_t *out);
/* From a problem handle: chained Rosenbrock, or the dense quadratic 1/2 x'Ax with ONE matrix A shared by
 * every instance (one matrix per instance: dzo_bfgs_batch_create_problem_matrices below); the decorators set on the handle (dzo_problem_set_l2 / set_box_gradient /
 * set_box_constraint, legacy/DZOptimization.jl:219-296) are applied inside the step kernel.  device < 0:
 * the device the calling thread selected (dzo_init). */
int32_t dzo_bfgs_batch_create_problem(dzo_problem_t problem, int64_t batch, const void *x0_dev,
                                      double initial_step_length, int32_t device, dzo_bfgs_batch_t *out);
/* The same with a DIFFERENT quadratic per instance ("run multiple optimizers in parallel", README.md:12, each with its own
 * objective): the handle gives kind (DZO_PROBLEM_QUADRATIC), n, dtype and the decorators; instance b minimises
 * 1/2 x'A_b x with A_b the symmetric n x n column-major matrix at matrices_dev + b * matrix_stride ELEMENTS
 * (matrix_stride >= n*n).  The caller owns matrices_dev and keeps it alive and unchanged while the batch exists. */
int32_t dzo_bfgs_batch_create_problem_matrices(dzo_problem_t problem, int64_t batch, const void *matrices_dev,
                                               int64_t matrix_stride, const void *x0_dev,
                                               double initial_step_length, int32_t device, dzo_bfgs_batch_t *out);
/* QuadraticLineSearch.max_increases (legacy/DZOptimization.jl:181-188, :138-151) of every instance; 0 = no cap */
int32_t dzo_bfgs_batch_set_max_increases(dzo_bfgs_batch_t b, int32_t max_increases);
int32_t dzo_bfgs_batch_destroy(dzo_bfgs_batch_t b);
/* runs `steps` synchronous step! calls on every live instance; *all_done = 1 when every
 * instance has_terminated.  Does not block unless all_done is non-NULL. */
int32_t dzo_bfgs_batch_step(dzo_bfgs_batch_t b, int32_t steps, int32_t *all_done);
/* get_ptr: 0 x (B x n) 1 g 2 H (B x n x n col-major) 3 f (B doubles) 4 has_terminated (B int32)
 *          5 iteration_count (B int64) 6 delta_point 7 delta_gradient 8 d 9 last_step_length
 *          10 last_step_type (B int32) */
int32_t dzo_bfgs_batch_get_ptr(dzo_bfgs_batch_t b, int32_t what, void **ptr_dev);
int32_t dzo_bfgs_batch_count_active(dzo_bfgs_batch_t b, int64_t *active);
/* The arrays behind dzo_bfgs_batch_get_ptr ARE the state of the instances (x, g, H, d, delta_point,
 * delta_gradient, f, last_step_length, last_step_type, has_terminated, iteration_count): writing them
 * between two dzo_bfgs_batch_step calls installs state (checkpoint / resume, README.md:11; the per-step
 * parity tests upload the CPU reference's state that way). */

/* The same constructor on an explicit device, for a host that drives the shards of several GPUs from
 * one process (dzo_comm_init_all).  x0_dev must live on `device`.  Every entry point of a batched
 * handle enters the handle's device by itself. */
int32_t dzo_bfgs_batch_create_on(int32_t device, int32_t problem_kind, int64_t batch, int64_t n, int32_t dtype,
                                 const void *x0_dev, double initial_step_length, dzo_bfgs_batch_t *out);
int32_t dzo_bfgs_batch_device(dzo_bfgs_batch_t b, int32_t *device);

/* ---------------------------------------------------------------------------------------
 * The one collective: the global convergence flag of sharded independent optimizers
 * (block partition of instances over the GPUs of a node, no data-path collective;
 * "run multiple optimizers in parallel", README.md:12).  all-reduce(MIN) of one int32 per rank over
 * RCCL / xGMI.  RCCL is loaded with dlopen at first use (no link-time dependency).
 *   dzo_comm_init_all   one process, several devices (ncclCommInitAll): local rank i = devices[i]
 *   dzo_comm_unique_id + dzo_comm_init_rank
 *                       one process per GPU: rank 0 creates the 128-byte id, the launcher carries
 *                       it to the other ranks, every rank joins with the device it selected (dzo_init)
 *   dzo_flag_allreduce_min   local_flags: one int32 per LOCAL rank; blocking
 *   dzo_flag_allreduce_min_n the same with the number of flags passed: DZO_ERR_INVALID unless it equals the
 *                       communicator's local rank count (what bindings with sized arrays should call)
 *   dzo_bfgs_batch_all_done  counts the live instances of every local shard (concurrently), then one
 *                       all-reduce: *all_done = 1 when every instance of every shard has_terminated.
 *                       comm may be NULL (no collective); otherwise batches[i] must live on the
 *                       device of local rank i.
 * ------------------------------------------------------------------------------------- */
#define DZO_COMM_UNIQUE_ID_BYTES 128
int32_t dzo_comm_unique_id(void *id128);
int32_t dzo_comm_init_rank(const void *id128, int32_t nranks, int32_t rank, dzo_comm_t *out);
int32_t dzo_comm_init_all(const int32_t *devices, int32_t ndev, dzo_comm_t *out);
int32_t dzo_comm_destroy(dzo_comm_t comm);
/* any of the outputs may be NULL; collectives = all-reduces issued so far */
int32_t dzo_comm_info(dzo_comm_t comm, int32_t *nranks, int32_t *nlocal, int32_t *first_rank, int64_t *collectives);
int32_t dzo_flag_allreduce_min(dzo_comm_t comm, const int32_t *local_flags, int32_t *global_flag);
int32_t dzo_flag_allreduce_min_n(dzo_comm_t comm, const int32_t *local_flags, int32_t nflags, int32_t *global_flag);
int32_t dzo_bfgs_batch_all_done(dzo_comm_t comm_or_null, const dzo_bfgs_batch_t *batches, int32_t nbatches,
                                int32_t *all_done);

#ifdef __cplusplus
}
#endif
#endif /* DZO_H */
