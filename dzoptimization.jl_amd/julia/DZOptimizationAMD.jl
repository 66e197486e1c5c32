# DZOptimizationAMD.jl -- Julia host module over the C ABI of include/dzo.h (libdzo_hip.so).
#
# Drop-in for the in-place BFGS / L-BFGS `step!()` path of dzhang314/DZOptimization.jl on an
# AMD MI355X: the same constructors, the same public fields, `step!`, and the termination flag
# under its three historical names (`is_stuck` live src/DZOptimization.jl:327, `has_terminated`
# legacy/DZOptimization.jl:478,738, `has_converged` README.md:38).  No CUDA.jl, no AMDGPU.jl:
# device memory and kernels live behind `ccall`.
#
# NOT EXERCISED IN THE BUILD CONTAINER (there is no Julia there); the tested twin of this file
# is the Python module next to it, which binds the very same symbols with ctypes.  Keep this
# file thin enough to be correct by inspection: every method is one ccall.
#
#   using DZOptimizationAMD
#   x   = HipVector(rand(10_000_000))
#   opt = LBFGSOptimizer(nothing, RosenbrockChain(length(x)), nothing, x, 1.0, 20)
#   while !opt.is_stuck[]; step!(opt); end
module DZOptimizationAMD

using LinearAlgebra
import LinearAlgebra: axpy!, axpby!, dot, norm, rmul!

export HipVector, LBFGSOptimizer, BFGSOptimizer, AdGDOptimizer, GradientDescentOptimizer, QuadraticLineSearch,
       UniformBoxConstraint, with_l2!, with_box_gradient!, with_box_constraint!, step!,
       set_safeguards!, set_line_search!, BACKTRACKING, STRONG_WOLFE,
       RosenbrockChain, Rosenbrock2D, DenseQuadratic, LogSumExp, QuadraticChain, BuiltinProblem,
       BatchedBFGSOptimizer, count_active, LineSearchEvaluator, compute_lbfgs_step_direction!,
       update_inverse_hessian!, reset_inverse_hessian!, synchronize,
       norm2, inv_norm, negate!, scale!, HipBackend, install_state!, ShardComm, all_done, read_field,
       lj_energy, lj_first_derivative, lj_second_derivative, PairwiseLennardJones,
       DZO_RADIAL_LENNARD_JONES, DZO_RADIAL_MORSE_RHO6, DZO_RADIAL_MORSE_RHO14,
       accelerated_pairwise_radial_energy, accelerated_pairwise_radial_gradient!, accelerated_pairwise_radial_hvp!,
       pairwise_radial_energy_delta,
       ParallelTempering, parallel_temper!, parallel_swap!, run_batches!, analyze, perturbation_radii,
       BatchedLBFGSOptimizer, BatchedAdGDOptimizer, current_step_sizes, count_active, objective_values, iteration_counts, stuck_flags, quench, pairwise_batch_energy_gradient!,
       pairwise_batch_hvp!, pairwise_batch_hessian!, symmetric_batch_eigen!, symeig_plan, hessian_spectrum,
       lowest_modes, LOWMODE_CONVERGED, LOWMODE_UNFINISHED, LOWMODE_FAILED,
       ModeFollowing, modefollow_apply!, set_start_mode!, set_directions!, polish_minima, find_saddles, read_array,
       HybridModeFollowing, hybridef_apply!, find_saddles_hybrid, HYBRIDEF_ACTIVE, HYBRIDEF_CONVERGED, HYBRIDEF_FAILED,
       structure_fingerprints, classify_structures, connect_saddles,
       ElasticBand, interpolate_band!, neb_apply!, neb_plan, connect_minima, NEB_ACTIVE, NEB_CONVERGED, NEB_FAILED,
       assign_particles, align_pairs, ALIGN_TRIAL_IDENTITY, ALIGN_TRIAL_PRINCIPAL, ALIGN_CONVERGED, ALIGN_CYCLE_LIMIT, ALIGN_FAILED,
       band_candidates, PATHWAY_MAX_BATCH, PATHWAY_OVERFLOW,
       BasinHopping, hop!, set_record!, set_array!,
       SphereLBFGS, sphere_project!, sphere_energy_gradient, DZO_SPHERE_ENERGY_RIESZ1

const libdzo = get(ENV, "DZO_LIB", joinpath(@__DIR__, "..", "libdzo_hip.so"))

const DZO_F32, DZO_F64 = Cint(0), Cint(1)
dtype_code(::Type{Float32}) = DZO_F32
dtype_code(::Type{Float64}) = DZO_F64

struct DzoError <: Exception
    code::Int
    msg::String
end

function check(rc::Integer)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:dzo_last_error, libdzo), Cstring, ()))
    rc == 3 && throw(AssertionError(msg))          # the reference's @assert
    throw(DzoError(rc, msg))
end

const _initialised = Ref(false)
function init(device::Integer=0)
    check(ccall((:dzo_init, libdzo), Cint, (Cint,), device))
    _initialised[] = true
end
ensure_init() = _initialised[] || init(parse(Int, get(ENV, "DZO_DEVICE", "0")))
"""Wait for every stream of the library (step functions return before their last kernels finish)."""
synchronize() = check(ccall((:dzo_synchronize, libdzo), Cint, ()))
"""Diagnostic (include/dzo.h): how often a host wait found a kernel's published result not yet matching its seal."""
function unsealed_first_reads()
    r = Ref{Int64}(0)
    check(ccall((:dzo_unsealed_first_reads, libdzo), Cint, (Ref{Int64},), r))
    return r[]
end

################################################################################ HipVector

"""Dense device vector: the array type `A<:AbstractArray{T}` the reference's optimizers are
generic over (src/DZOptimization.jl:101,179,321)."""
mutable struct HipVector{T<:Union{Float32,Float64}} <: AbstractVector{T}
    ptr::Ptr{Cvoid}
    len::Int
    owner::Bool
    function HipVector{T}(::UndefInitializer, n::Integer) where {T}
        ensure_init()
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:dzo_malloc, libdzo), Cint, (Ref{Ptr{Cvoid}}, Int64), p, max(n * sizeof(T), 16)))
        v = new{T}(p[], n, true)
        finalizer(v) do w
            w.owner && w.ptr != C_NULL && ccall((:dzo_free, libdzo), Cint, (Ptr{Cvoid},), w.ptr)
            w.ptr = C_NULL
        end
        return v
    end
    HipVector{T}(p::Ptr{Cvoid}, n::Integer) where {T} = new{T}(p, n, false)   # borrowed view
end

function HipVector(a::AbstractArray{T}) where {T<:Union{Float32,Float64}}
    v = HipVector{T}(undef, length(a))
    h = Array{T}(vec(a))
    check(ccall((:dzo_memcpy_h2d, libdzo), Cint, (Ptr{Cvoid}, Ptr{T}, Int64), v.ptr, h, sizeof(h)))
    return v
end

Base.size(v::HipVector) = (v.len,)
Base.length(v::HipVector) = v.len
Base.similar(v::HipVector{T}) where {T} = HipVector{T}(undef, v.len)
Base.getindex(v::HipVector, i::Int) = Array(v)[i]          # debugging only: one D2H per call
function Base.Array(v::HipVector{T}) where {T}
    h = Vector{T}(undef, v.len)
    check(ccall((:dzo_memcpy_d2h, libdzo), Cint, (Ptr{T}, Ptr{Cvoid}, Int64), h, v.ptr, sizeof(h)))
    return h
end
function Base.copy!(dst::HipVector{T}, src::HipVector{T}) where {T}
    check(ccall((:dzo_copy, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}), src.len, dtype_code(T), src.ptr, dst.ptr))
    return dst
end
Base.copy(v::HipVector) = copy!(similar(v), v)
function Base.fill!(v::HipVector{T}, a) where {T}
    check(ccall((:dzo_fill, libdzo), Cint, (Int64, Cint, Cdouble, Ptr{Cvoid}), v.len, dtype_code(T), Float64(a), v.ptr))
    return v
end
function Base.isequal(a::HipVector{T}, b::HipVector{T}) where {T}
    r = Ref{Cint}(0)
    check(ccall((:dzo_isequal, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cint}), a.len, dtype_code(T), a.ptr, b.ptr, r))
    return r[] != 0
end

# the L1 method set the reference calls (src/DZOptimization.jl:4)
function axpy!(a::Number, x::HipVector{T}, y::HipVector{T}) where {T}
    check(ccall((:dzo_axpy, libdzo), Cint, (Int64, Cint, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}), x.len, dtype_code(T), Float64(a), x.ptr, y.ptr))
    return y
end
function axpby!(a::Number, x::HipVector{T}, b::Number, y::HipVector{T}) where {T}
    check(ccall((:dzo_axpby, libdzo), Cint, (Int64, Cint, Cdouble, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}), x.len, dtype_code(T), Float64(a), x.ptr, Float64(b), y.ptr))
    return y
end
function rmul!(x::HipVector{T}, a::Number) where {T}
    check(ccall((:dzo_scal, libdzo), Cint, (Int64, Cint, Cdouble, Ptr{Cvoid}), x.len, dtype_code(T), Float64(a), x.ptr))
    return x
end
function dot(x::HipVector{T}, y::HipVector{T}) where {T}
    r = Ref{Cdouble}(0)
    check(ccall((:dzo_dot, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}), x.len, dtype_code(T), x.ptr, y.ptr, r))
    return T(r[])
end
function norm(x::HipVector{T}) where {T}
    r = Ref{Cdouble}(0)
    check(ccall((:dzo_nrm2, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ref{Cdouble}), x.len, dtype_code(T), x.ptr, r))
    return T(r[])
end

# legacy/Kernels.jl primitives without a LinearAlgebra twin (SURVEY.md a14)
"""`norm2(x)`: the sum of squares, NOT its root (legacy/Kernels.jl:49-55,139)."""
function norm2(x::HipVector{T}) where {T}
    r = Ref{Cdouble}(0)
    check(ccall((:dzo_norm2, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ref{Cdouble}), x.len, dtype_code(T), x.ptr, r))
    return T(r[])
end
"""`inv_norm(x) = rsqrt(norm2(x))` (legacy/Kernels.jl:141)."""
function inv_norm(x::HipVector{T}) where {T}
    r = Ref{Cdouble}(0)
    check(ccall((:dzo_inv_norm, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ref{Cdouble}), x.len, dtype_code(T), x.ptr, r))
    return T(r[])
end
"""`negate!(x)` (legacy/Kernels.jl:76-83,143)."""
function negate!(x::HipVector{T}) where {T}
    check(ccall((:dzo_negate, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}), x.len, dtype_code(T), x.ptr))
    return x
end
"""`scale!(x, alpha)` in place (legacy/Kernels.jl:87-94,145-146), `scale!(dst, alpha, x)` out of place (:96-104)."""
scale!(x::HipVector, alpha::Number) = rmul!(x, alpha)
function scale!(dst::HipVector{T}, alpha::Number, x::HipVector{T}) where {T}
    check(ccall((:dzo_scal_oop, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}), x.len, dtype_code(T), dst.ptr, Float64(alpha), x.ptr))
    return x                                                   # (the reference returns x, :103)
end

# KernelAbstractions.get_backend(::HipVector): the reference's constructors call it on every array and
# @assert the backends equal (src/DZOptimization.jl:3,44-54,216-226,363-378,410,420).  KernelAbstractions
# is a dependency of the REFERENCE, not of this module: when it is loadable (it is whenever the
# reference itself is), HipVector gets a singleton backend, so the reference's own generic
# constructors and `step!` run unmodified on HipVector (INTEGRATION.md route A).
const _KA = try
    Base.require(Base.PkgId(Base.UUID("63c18a36-062a-441e-b654-da1e3ab1ce7c"), "KernelAbstractions"))
catch
    nothing
end
if _KA !== nothing
    @eval begin
        """Singleton backend of `HipVector` (device memory behind libdzo_hip.so)."""
        struct HipBackend <: $(_KA).GPU end
        $(_KA).get_backend(::HipVector) = HipBackend()
    end
else
    struct HipBackend end                                       # KernelAbstractions absent: route B only
end

################################################################################ built-in objectives

mutable struct BuiltinProblem{T}
    handle::Ptr{Cvoid}
    n::Int
    keep::Any
    function BuiltinProblem{T}(h::Ptr{Cvoid}, n::Integer, keep) where {T}
        # optimizers built from a problem hold it in a field, so it outlives their handles
        return finalizer(q -> ccall((:dzo_problem_destroy, libdzo), Cint, (Ptr{Cvoid},), q.handle), new{T}(h, n, keep))
    end
end
function _problem(kind, n, ::Type{T}; A=nothing, c=nothing, lambda=0.0) where {T}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_problem_create, libdzo), Cint,
                (Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                kind, n, dtype_code(T), A === nothing ? C_NULL : A.ptr, c === nothing ? C_NULL : c.ptr, lambda, h))
    return BuiltinProblem{T}(h[], n, (A, c))
end
Rosenbrock2D(::Type{T}=Float64) where {T} = _problem(0, 2, T)
RosenbrockChain(n::Integer, ::Type{T}=Float64) where {T} = _problem(1, n, T)
DenseQuadratic(A::HipVector{T}, n::Integer) where {T} = _problem(2, n, T; A=A)      # A column-major n*n
LogSumExp(c::HipVector{T}, lambda) where {T} = _problem(3, length(c), T; c=c, lambda=lambda)
# sum 1/2 (x[i+1]-x[i])^2 + lambda/2 (x[i]-1)^2: the large-n convex quadratic (tridiagonal Hessian); like RosenbrockChain it runs on
# the L-BFGS point pass (DZO_PROBLEM_QUADRATIC_CHAIN)
QuadraticChain(n::Integer, lambda, ::Type{T}=Float64) where {T} = _problem(4, n, T; lambda=lambda)
# the pairwise Lennard-Jones objective of src/ExampleFunctions.jl on the point [x | y | z], n = 3N (DZO_PROBLEM_PAIRWISE_LJ)
PairwiseLennardJones(n_particles::Integer, ::Type{T}=Float64) where {T} = _problem(5, 3 * n_particles, T)
function (p::BuiltinProblem{T})(x::HipVector{T}) where {T}                           # objective_function(x)
    f = Ref{Cdouble}(0)
    check(ccall((:dzo_problem_eval, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}), p.handle, x.ptr, f))
    return T(f[])
end
function gradient!(p::BuiltinProblem{T}, g::HipVector{T}, x::HipVector{T}) where {T}
    check(ccall((:dzo_problem_grad, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), p.handle, g.ptr, x.ptr))
    return g
end

################################################################################ pairwise radial functions (src/ExampleFunctions.jl)

@inline _twice(x) = x + x
@inline _square(x) = x * x
# The radial functions as host functions, operation by operation what the reference defines (:16-72); on HipVector
# arguments the accelerated_* methods below dispatch on their TYPES to the device kernels that evaluate the same arithmetic.
@inline function lj_energy(r2::T) where {T}
    inv_r2 = inv(r2); inv_r4 = _square(inv_r2); inv_r6 = inv_r4 * inv_r2
    return T(4) * muladd(inv_r6, inv_r6, -inv_r6)
end
@inline function lj_first_derivative(r2::T) where {T}
    inv_r2 = inv(r2); inv_r4 = _square(inv_r2); inv_r6 = inv_r4 * inv_r2; inv_r8 = _square(inv_r4)
    return T(-12) * muladd(inv_r8, _twice(inv_r6), -inv_r8)
end
@inline function lj_second_derivative(r2::T) where {T}
    inv_r2 = inv(r2); inv_r4 = _square(inv_r2); inv_r8 = _square(inv_r4); inv_r10 = inv_r8 * inv_r2
    return T(48) * muladd(T(7) / T(2), _square(inv_r8), -inv_r10)
end
const DZO_RADIAL_LENNARD_JONES = Cint(0)
# E(r) = t^2 - 2 t, t = exp(rho (1 - r)): pair minimum at r = 1, depth 1; rho is compile-time in the library (include/dzo.h).
# Every function below that reaches a radial takes `radial=` (the Lennard-Jones selector by default).
const DZO_RADIAL_MORSE_RHO6 = Cint(2)
const DZO_RADIAL_MORSE_RHO14 = Cint(3)

"""`accelerated_pairwise_radial_energy(lj_energy, x, y, z)` on device vectors (src/ExampleFunctions.jl:152-173)."""
function accelerated_pairwise_radial_energy(::typeof(lj_energy), x::HipVector{T}, y::HipVector{T}, z::HipVector{T}; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    e = Ref{Cdouble}(0)
    check(ccall((:dzo_pairwise_energy, libdzo), Cint, (Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}),
                Cint(radial), x.len, dtype_code(T), x.ptr, y.ptr, z.ptr, e))
    return T(e[])
end
"""`accelerated_pairwise_radial_gradient!(gx, gy, gz, lj_first_derivative, x, y, z)` (src/ExampleFunctions.jl:265-294)."""
function accelerated_pairwise_radial_gradient!(gx::HipVector{T}, gy::HipVector{T}, gz::HipVector{T}, ::typeof(lj_first_derivative),
                                               x::HipVector{T}, y::HipVector{T}, z::HipVector{T}; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    check(ccall((:dzo_pairwise_gradient, libdzo), Cint,
                (Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), x.len, dtype_code(T), gx.ptr, gy.ptr, gz.ptr, x.ptr, y.ptr, z.ptr))
    return nothing
end
"""`accelerated_pairwise_radial_hvp!(px, py, pz, lj_first_derivative, lj_second_derivative, x, y, z, u, v, w)` (:427-468)."""
function accelerated_pairwise_radial_hvp!(px::HipVector{T}, py::HipVector{T}, pz::HipVector{T}, ::typeof(lj_first_derivative),
                                          ::typeof(lj_second_derivative), x::HipVector{T}, y::HipVector{T}, z::HipVector{T},
                                          u::HipVector{T}, v::HipVector{T}, w::HipVector{T}; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    check(ccall((:dzo_pairwise_hvp, libdzo), Cint,
                (Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), x.len, dtype_code(T), px.ptr, py.ptr, pz.ptr, x.ptr, y.ptr, z.ptr, u.ptr, v.ptr, w.ptr))
    return nothing
end
"""`pairwise_radial_energy_delta(lj_energy, x, y, z, i, x_new, y_new, z_new)` (:477-534); `i` is 1-based like the reference's."""
function pairwise_radial_energy_delta(::typeof(lj_energy), x::HipVector{T}, y::HipVector{T}, z::HipVector{T}, i::Integer,
                                      x_new::Real, y_new::Real, z_new::Real; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    d = Ref{Cdouble}(0)
    check(ccall((:dzo_pairwise_energy_delta, libdzo), Cint,
                (Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cdouble, Cdouble, Cdouble, Ref{Cdouble}),
                Cint(radial), x.len, dtype_code(T), x.ptr, y.ptr, z.ptr, i - 1, Float64(x_new), Float64(y_new), Float64(z_new), d))
    return T(d[])
end

################################################################################ parallel tempering (scripts/MonteCarlo.jl)
# NOT EXERCISED IN THE BUILD CONTAINER (no Julia there), like the rest of this file; tests/test_abi.py checks every ccall
# below against include/dzo.h, and the Python class ParallelTempering binds the same ten entry points and IS tested.
#
# The reference's functions take everything per call; what outlives a call here (the device copies of the inverse
# temperatures and perturbation radii, the random streams of include/dzo.h's rule) lives in the handle.  `replicas` is the
# reference's Array{T,3}(particles, 3, replicas) as one device vector, aliased and mutated.  Julia's rand / randn streams are
# not reproduced: a run agrees with the script's in distribution only.

mutable struct ParallelTempering{T}
    handle::Ptr{Cvoid}
    replicas::HipVector{T}
    n_particles::Int
    n_replicas::Int
end

"""`ParallelTempering(lj_energy, replicas, n_particles, inverse_temperatures, perturbation_radii, constraining_radius; seed)`:
the arguments of `parallel_temper!` (scripts/MonteCarlo.jl:8-15)."""
function ParallelTempering(::typeof(lj_energy), replicas::HipVector{T}, n_particles::Integer, inverse_temperatures::AbstractVector,
                           perturbation_radii::AbstractVector, constraining_radius::Real; seed::Integer=0, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    n_replicas = length(inverse_temperatures)
    @assert length(perturbation_radii) == n_replicas                       # :33
    @assert length(replicas) == 3 * n_particles * n_replicas               # :31
    beta = Vector{Cdouble}(inverse_temperatures); radii = Vector{Cdouble}(perturbation_radii)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_tempering_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, UInt64, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, n_replicas, dtype_code(T), replicas.ptr, beta, radii, Float64(constraining_radius), UInt64(seed), h))
    pt = ParallelTempering{T}(h[], replicas, n_particles, n_replicas)
    finalizer(pt) do w
        w.handle != C_NULL && ccall((:dzo_tempering_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return pt
end

"""`parallel_temper!(pt, energies, num_steps; ld)` (scripts/MonteCarlo.jl:8-86): `energies[i + ld * k]`, 0-based, is the energy
of replica k after move i.  Does not block."""
function parallel_temper!(pt::ParallelTempering{T}, energies::HipVector{T}, num_steps::Integer; ld::Integer=num_steps) where {T}
    check(ccall((:dzo_tempering_temper, libdzo), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64), pt.handle, num_steps, energies.ptr, ld))
    return nothing
end

"""`parallel_swap!(pt, odd)` (scripts/MonteCarlo.jl:89-136).  Does not block."""
function parallel_swap!(pt::ParallelTempering, odd::Bool)
    check(ccall((:dzo_tempering_swap, libdzo), Cint, (Ptr{Cvoid}, Cint), pt.handle, odd ? 1 : 0))
    return nothing
end

"""`run_batches!(pt, energies, num_steps, num_batches; ld)`: the loop body of `main` (scripts/MonteCarlo.jl:222-231)."""
function run_batches!(pt::ParallelTempering{T}, energies::HipVector{T}, num_steps::Integer, num_batches::Integer;
                      ld::Integer=2 * num_steps * num_batches) where {T}
    check(ccall((:dzo_tempering_run, libdzo), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64), pt.handle, num_steps, num_batches, energies.ptr, ld))
    return nothing
end

"""`analyze(pt, energies, n_iterations; ld)` (scripts/MonteCarlo.jl:139-180): `(cv, cv_prime)` as host vectors of T."""
function analyze(pt::ParallelTempering{T}, energies::HipVector{T}, n_iterations::Integer; ld::Integer=n_iterations) where {T}
    cv = Vector{Cdouble}(undef, pt.n_replicas); cv_prime = Vector{Cdouble}(undef, pt.n_replicas)
    check(ccall((:dzo_tempering_analyze, libdzo), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                pt.handle, n_iterations, energies.ptr, ld, cv, cv_prime, C_NULL))
    return Vector{T}(cv), Vector{T}(cv_prime)
end

"""The perturbation radii after the adaptation of the last `parallel_temper!` (scripts/MonteCarlo.jl:77-81); blocks."""
function perturbation_radii(pt::ParallelTempering{T}) where {T}
    r = Vector{T}(undef, pt.n_replicas)
    check(ccall((:dzo_tempering_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), pt.handle, 1, r))
    return r
end

################################################################################ batched L-BFGS over Lennard-Jones clusters
# (not exercised in the build container either; the Python class BatchedLBFGS binds the same entry points and IS tested)
#
# The live LBFGSOptimizer (src/DZOptimization.jl:321-509, constraint_function! = nothing) of `batch` clusters of
# `n_particles` particles at once: `step!(opt, k)` runs k calls of the reference's step!() of every instance in ONE launch.
# `points` holds instance b as [x | y | z] at 3 n_particles b (the tempering replica layout); it is aliased (:393).

mutable struct BatchedLBFGSOptimizer{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
    history_length::Int
end

"""`BatchedLBFGSOptimizer(lj_energy, points, n_particles, initial_step_length, history_length)` (:400-427 per instance)."""
function BatchedLBFGSOptimizer(::typeof(lj_energy), points::HipVector{T}, n_particles::Integer, initial_step_length::Real,
                               history_length::Integer; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_lbfgs_batch_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, Float64(initial_step_length), history_length, h))
    opt = BatchedLBFGSOptimizer{T}(h[], points, n_particles, batch, history_length)
    finalizer(opt) do w
        w.handle != C_NULL && ccall((:dzo_lbfgs_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return opt
end

"""`step!(opt, steps; wait=true)`: `steps` calls of step!() (:454-509) of every instance that is not stuck, one launch.
Returns whether every instance is stuck (`wait=true`, blocking) or `nothing` (enqueued only)."""
function step!(opt::BatchedLBFGSOptimizer, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_lbfgs_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), opt.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_lbfgs_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), opt.handle, steps, flag))
    return flag[] != 0
end

"""The bound on the halvings of one step (the project's escape from the loop of :121-153; default 4096)."""
set_max_halvings!(opt::BatchedLBFGSOptimizer, v::Integer) =
    (check(ccall((:dzo_lbfgs_batch_set_max_halvings, libdzo), Cint, (Ptr{Cvoid}, Int64), opt.handle, v)); opt)

function count_active(opt::BatchedLBFGSOptimizer)
    n = Ref{Int64}(0)
    check(ccall((:dzo_lbfgs_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), opt.handle, n))
    return Int(n[])
end

"""current_objective_value of every instance (DZO_LBFGS_BATCH_OBJECTIVES); blocks."""
function objective_values(opt::BatchedLBFGSOptimizer{T}) where {T}
    r = Vector{T}(undef, opt.batch)
    check(ccall((:dzo_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 5, r))
    return r
end

"""iteration_count of every instance (DZO_LBFGS_BATCH_ITERATION_COUNTS); blocks."""
function iteration_counts(opt::BatchedLBFGSOptimizer)
    r = Vector{Int64}(undef, opt.batch)
    check(ccall((:dzo_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 8, r))
    return r
end

"""is_stuck of every instance (DZO_LBFGS_BATCH_IS_STUCK); blocks."""
function stuck_flags(opt::BatchedLBFGSOptimizer)
    r = Vector{Int32}(undef, opt.batch)
    check(ccall((:dzo_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 7, r))
    return r .!= 0
end

"""Device address of one of the DZO_LBFGS_BATCH_* arrays of include/dzo.h (no wait)."""
function array_pointer(opt::BatchedLBFGSOptimizer, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_lbfgs_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), opt.handle, what, p))
    return p[]
end

"""`pairwise_batch_energy_gradient!(energies, gradients, points, n_particles)`: energy and gradient of every instance by the
optimizer's own device routine (the objective_function / gradient_function! of :416-421); blocks."""
function pairwise_batch_energy_gradient!(energies::HipVector{T}, gradients::HipVector{T}, points::HipVector{T}, n_particles::Integer; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    check(ccall((:dzo_pairwise_batch_energy_gradient, libdzo), Cint, (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, energies.ptr, gradients.ptr))
    return energies
end

################################################################################ the Thomson problem: Riesz energy on the unit sphere
# (not exercised in the build container either; the Python class SphereLBFGS binds the same entry points and IS tested)
#
# The live LBFGSOptimizer WITH its constraint hook (constraint_function!, :133-135 and :412-414) on the reference author's own
# example objective, riesz_energy / riesz_gradient! / constrain_riesz_gradient_sphere! of legacy/ExampleFunctions.jl (:30-45,
# :47-83, :361-374), of `batch` configurations of `n_particles` charges at once.  `points` holds instance b as [x | y | z] at
# 3 n_particles b (the legacy functions take a (3, N) matrix); it is aliased (:393) and projected in place (:412-414).

const DZO_SPHERE_ENERGY_RIESZ1 = 0

"""`sphere_project!(points, n_particles)`: every particle of every instance divided by its norm, in place; blocks."""
function sphere_project!(points::HipVector{T}, n_particles::Integer) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    check(ccall((:dzo_sphere_batch_project, libdzo), Cint, (Int64, Int64, Cint, Ptr{Cvoid}),
                n_particles, batch, dtype_code(T), points.ptr))
    return points
end

"""`sphere_energy_gradient(energies, gradients, points, n_particles; tangent=true)`: the Riesz (s = 1) energy of every instance and,
unless `gradients === nothing`, its gradient: raw (`riesz_gradient!`) or, with `tangent`, after
`constrain_riesz_gradient_sphere!`; by the optimizer's own device routine.  Blocks."""
function sphere_energy_gradient(energies::HipVector{T}, gradients::Union{Nothing,HipVector{T}}, points::HipVector{T}, n_particles::Integer;
                                tangent::Bool=true) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    @assert length(energies) == batch
    @assert gradients === nothing || length(gradients) == length(points)
    check(ccall((:dzo_sphere_batch_energy_gradient, libdzo), Cint, (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint),
                Cint(DZO_SPHERE_ENERGY_RIESZ1), n_particles, batch, dtype_code(T), points.ptr, energies.ptr,
                gradients === nothing ? C_NULL : gradients.ptr, Cint(tangent)))
    return energies
end

mutable struct SphereLBFGS{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
    history_length::Int
end

"""`SphereLBFGS(points, n_particles, initial_step_length, history_length)` (:400-427 per instance, the unit sphere as constraint)."""
function SphereLBFGS(points::HipVector{T}, n_particles::Integer, initial_step_length::Real, history_length::Integer) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_sphere_lbfgs_batch_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                Cint(DZO_SPHERE_ENERGY_RIESZ1), n_particles, batch, dtype_code(T), points.ptr, Float64(initial_step_length), history_length, h))
    opt = SphereLBFGS{T}(h[], points, n_particles, batch, history_length)
    finalizer(opt) do w
        w.handle != C_NULL && ccall((:dzo_sphere_lbfgs_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return opt
end

function step!(opt::SphereLBFGS, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_sphere_lbfgs_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), opt.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_sphere_lbfgs_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), opt.handle, steps, flag))
    return flag[] != 0
end

set_max_halvings!(opt::SphereLBFGS, v::Integer) =
    (check(ccall((:dzo_sphere_lbfgs_batch_set_max_halvings, libdzo), Cint, (Ptr{Cvoid}, Int64), opt.handle, v)); opt)

function count_active(opt::SphereLBFGS)
    n = Ref{Int64}(0)
    check(ccall((:dzo_sphere_lbfgs_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), opt.handle, n))
    return Int(n[])
end

"""current_objective_value of every instance (DZO_LBFGS_BATCH_OBJECTIVES); blocks."""
function objective_values(opt::SphereLBFGS{T}) where {T}
    r = Vector{T}(undef, opt.batch)
    check(ccall((:dzo_sphere_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 5, r))
    return r
end

"""iteration_count of every instance (DZO_LBFGS_BATCH_ITERATION_COUNTS); blocks."""
function iteration_counts(opt::SphereLBFGS)
    r = Vector{Int64}(undef, opt.batch)
    check(ccall((:dzo_sphere_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 8, r))
    return r
end

"""is_stuck of every instance (DZO_LBFGS_BATCH_IS_STUCK): with the gradient, what tells a minimum from a step without descent; blocks."""
function stuck_flags(opt::SphereLBFGS)
    r = Vector{Int32}(undef, opt.batch)
    check(ccall((:dzo_sphere_lbfgs_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, 7, r))
    return r .!= 0
end

"""Device address of one of the DZO_LBFGS_BATCH_* arrays of include/dzo.h (no wait)."""
function array_pointer(opt::SphereLBFGS, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_sphere_lbfgs_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), opt.handle, what, p))
    return p[]
end

"""`pairwise_batch_hvp!(products, points, directions, n_particles; curvatures=nothing, shared_point=false)`:
accelerated_pairwise_radial_hvp! (src/ExampleFunctions.jl:367-468) of every instance in one launch.  `curvatures`: a
`HipVector{Float64}` of 2 * batch elements for u.Hu and u.u of each instance.  `shared_point`: `points` holds one point to which
every direction is applied.  Blocks."""
function pairwise_batch_hvp!(products::HipVector{T}, points::HipVector{T}, directions::HipVector{T}, n_particles::Integer;
                             curvatures::Union{Nothing,HipVector{Float64}}=nothing, shared_point::Bool=false, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(directions), 3 * n_particles)
    check(ccall((:dzo_pairwise_batch_hvp, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, shared_point ? 0 : 3 * n_particles,
                directions.ptr, products.ptr, curvatures === nothing ? C_NULL : curvatures.ptr))
    return products
end

"""`pairwise_batch_hessian!(hessians, points, n_particles)`: the dense 3N x 3N Hessian of every instance, column-major per
instance (`reshape(Array(hessians), 3N, 3N, batch)`), from one launch.  Blocks."""
function pairwise_batch_hessian!(hessians::HipVector{T}, points::HipVector{T}, n_particles::Integer; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    check(ccall((:dzo_pairwise_batch_hessian, libdzo), Cint, (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, hessians.ptr))
    return hessians
end

"""`symmetric_batch_eigen!(eigenvalues, matrices, n; eigenvectors=nothing, max_sweeps=0)`: eigenvalues (ascending, n per
instance) and optionally eigenvectors (n x n per instance, column-major, column k belongs to eigenvalue k) of the symmetric part
of every n x n matrix of `matrices` (column-major per instance: what `pairwise_batch_hessian!` writes), by cyclic Jacobi on the
device, one launch.  Returns the sweeps each instance ran as a `Vector{Int32}`, -1 where `max_sweeps` (0: the default, 30) did
not suffice.  `matrices` is not modified.  Blocks."""
function symmetric_batch_eigen!(eigenvalues::HipVector{T}, matrices::HipVector{T}, n::Integer;
                                eigenvectors::Union{Nothing,HipVector{T}}=nothing, max_sweeps::Integer=0) where {T}
    batch = div(length(matrices), n * n)
    sweeps = HipVector{Float32}(undef, batch)               # four bytes per instance: read back as Int32
    check(ccall((:dzo_symmetric_batch_eigen, libdzo), Cint,
                (Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint),
                n, batch, dtype_code(T), matrices.ptr, eigenvalues.ptr, eigenvectors === nothing ? C_NULL : eigenvectors.ptr,
                sweeps.ptr, max_sweeps))
    return collect(reinterpret(Int32, Array(sweeps)))
end

"""`symeig_plan(n, T)`: `(storage, ld, lds_bytes)` -- where `symmetric_batch_eigen!` keeps an n x n matrix of `T` while it
iterates (0: LDS, 1: device memory), its leading dimension and the dynamic LDS of the launch.  A pure function; no device."""
function symeig_plan(n::Integer, ::Type{T}) where {T<:Union{Float32,Float64}}
    storage, ld, lds = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:dzo_symeig_plan, libdzo), Cint, (Int64, Cint, Ref{Cint}, Ref{Int64}, Ref{Int64}),
                n, dtype_code(T), storage, ld, lds))
    return Int(storage[]), Int(ld[]), Int(lds[])
end

"""`hessian_spectrum(points, n_particles)`: the eigenvalues of the Hessian of every instance as a `3N x batch` `Matrix{Float64}`,
ascending per column: `pairwise_batch_hessian!` into `symmetric_batch_eigen!` without leaving the device.  Throws when an
instance does not converge (a non-finite Hessian)."""
function hessian_spectrum(points::HipVector{T}, n_particles::Integer) where {T}
    n = 3 * n_particles
    batch = div(length(points), n)
    hessians = pairwise_batch_hessian!(HipVector{T}(undef, n * n * batch), points, n_particles)
    eigenvalues = HipVector{T}(undef, n * batch)
    sweeps = symmetric_batch_eigen!(eigenvalues, hessians, n)
    any(<(0), sweeps) && error("hessian_spectrum: no convergence in instances $(findall(<(0), sweeps))")
    return Float64.(reshape(Array(eigenvalues), n, batch))
end

const LOWMODE_CONVERGED, LOWMODE_UNFINISHED, LOWMODE_FAILED = Int32(0), Int32(1), Int32(2)

"""`lowest_modes(points, n_particles; project_rigid=true, krylov=32, max_cycles=40, res_tol=nothing, start=nothing, seed=0)`:
the lowest eigenpair of the Hessian of every instance by restarted Lanczos inside one launch (include/dzo.h, "Batched lowest
Hessian mode"): Hessian-vector products only, up to 1024 particles.  `project_rigid`: net translation and rotation are projected
out.  `res_tol === nothing`: 4.3e-15 for Float64, 7.0e-7 for Float32 (DESIGN.md).  `start`: start vectors laid out like `points`,
or `nothing` to draw them in the kernel from `seed`.  Returns `(eigenvalues::Vector{T}, vectors::HipVector{T}, residuals::Vector{Float64},
status, cycles, products)`, the last three `Vector{Int32}`.  Blocks."""
function lowest_modes(points::HipVector{T}, n_particles::Integer; project_rigid::Bool=true, krylov::Integer=32, max_cycles::Integer=40,
                      res_tol::Union{Nothing,Real}=nothing, start::Union{Nothing,HipVector{T}}=nothing, seed::Integer=0, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    tol = res_tol === nothing ? (T === Float64 ? 4.3e-15 : 7.0e-7) : Float64(res_tol)
    eigenvalues = HipVector{T}(undef, batch)
    vectors = HipVector{T}(undef, 3 * n_particles * batch)
    residuals = HipVector{Float64}(undef, batch)
    info = HipVector{Float32}(undef, 3 * batch)              # four bytes per record: read back as Int32
    check(ccall((:dzo_pairwise_batch_lowest_mode, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cint, Cint, Cint, Cdouble, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, project_rigid ? 1 : 0, krylov, max_cycles, tol,
                UInt64(seed), start === nothing ? C_NULL : start.ptr, eigenvalues.ptr, vectors.ptr, residuals.ptr, info.ptr))
    records = reshape(collect(reinterpret(Int32, Array(info))), 3, batch)
    return Array(eigenvalues), vectors, Array(residuals), records[1, :], records[2, :], records[3, :]
end

################################################################################ batched basin hopping
# (not exercised in the build container either; the Python class BasinHopping binds the same entry points and IS tested)
#
# Basin hopping (Wales & Doye 1997; include/dzo.h states the rule) of `batch` walkers at once: `hop!(bh, k)` runs k hops --
# perturb every particle, quench with the batched L-BFGS, Metropolis test on the quenched energies -- of every walker at the
# walker's own pace.  `points` is aliased and always holds the walkers' current minima.

# `what` of read_array / set_array! (DZO_BASIN_HOPPING_* of include/dzo.h)
const BASIN_HOPPING_POINTS, BASIN_HOPPING_ENERGIES, BASIN_HOPPING_BEST_POINTS, BASIN_HOPPING_BEST_ENERGIES, BASIN_HOPPING_RADII,
      BASIN_HOPPING_INV_TEMPS, BASIN_HOPPING_NUM_ACCEPT, BASIN_HOPPING_NUM_REJECT, BASIN_HOPPING_RNG_STATES, BASIN_HOPPING_HOP_COUNTS,
      BASIN_HOPPING_QUENCH_ITERATIONS, BASIN_HOPPING_QUENCH_UNFINISHED, BASIN_HOPPING_REC_NORMALS, BASIN_HOPPING_REC_UNIFORM,
      BASIN_HOPPING_REC_TRIAL_ENERGY, BASIN_HOPPING_REC_QUENCH_ITERATIONS, BASIN_HOPPING_REC_CODE = 0:16

mutable struct BasinHopping{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
    record_capacity::Int
end

"""`BasinHopping(lj_energy, points, n_particles, inverse_temperatures, perturbation_radii, constraining_radius;
initial_step_length=0.01, history_length=10, quench_steps=400, seed=0)`.  Does not wait for the quench of `points`."""
function BasinHopping(::typeof(lj_energy), points::HipVector{T}, n_particles::Integer, inverse_temperatures::AbstractVector,
                      perturbation_radii::AbstractVector, constraining_radius::Real; initial_step_length::Real=0.01,
                      history_length::Integer=10, quench_steps::Integer=400, seed::Integer=0, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = length(inverse_temperatures)
    @assert length(perturbation_radii) == batch
    @assert length(points) == 3 * n_particles * batch
    beta = Vector{Cdouble}(inverse_temperatures); radii = Vector{Cdouble}(perturbation_radii)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_basin_hopping_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cint, Cint, UInt64, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, beta, radii, Float64(constraining_radius),
                Float64(initial_step_length), history_length, quench_steps, UInt64(seed), h))
    bh = BasinHopping{T}(h[], points, n_particles, batch, 0)
    finalizer(bh) do w
        w.handle != C_NULL && ccall((:dzo_basin_hopping_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return bh
end

"""The bound on the halvings of one quench step (default 4096)."""
set_max_halvings!(bh::BasinHopping, max_halvings::Integer) =
    (check(ccall((:dzo_basin_hopping_set_max_halvings, libdzo), Cint, (Ptr{Cvoid}, Int64), bh.handle, max_halvings)); bh)

"""`hop!(bh, num_hops; adapt=true, hops_per_launch=8, wait=true)`: `cld(num_hops, hops_per_launch)` launches; the radii are
adapted (scripts/MonteCarlo.jl:77-81) at the end of the last one when `adapt` is set."""
function hop!(bh::BasinHopping, num_hops::Integer; adapt::Bool=true, hops_per_launch::Integer=8, wait::Bool=true)
    done = 0
    while done < num_hops
        k = min(hops_per_launch, num_hops - done)
        done += k
        check(ccall((:dzo_basin_hopping_hop, libdzo), Cint, (Ptr{Cvoid}, Int64, Cint), bh.handle, k, (adapt && done == num_hops) ? 1 : 0))
    end
    wait && synchronize()
    return bh
end

"""Record the draws and decisions of the hop calls that follow, up to `capacity_hops` hops per launch; 0 switches it off."""
function set_record!(bh::BasinHopping, capacity_hops::Integer)
    check(ccall((:dzo_basin_hopping_set_record, libdzo), Cint, (Ptr{Cvoid}, Int64), bh.handle, capacity_hops))
    bh.record_capacity = capacity_hops
    return bh
end

"""`read_array(bh, what)`: a blocking host copy of one of the BASIN_HOPPING_* arrays, in its own element type, the walker as
the last dimension."""
function read_array(bh::BasinHopping{T}, what::Integer) where {T}
    n, b, cap = bh.n_particles, bh.batch, bh.record_capacity
    r = what in (BASIN_HOPPING_POINTS, BASIN_HOPPING_BEST_POINTS) ? Array{T}(undef, 3 * n, b) :
        what in (BASIN_HOPPING_ENERGIES, BASIN_HOPPING_BEST_ENERGIES, BASIN_HOPPING_RADII, BASIN_HOPPING_INV_TEMPS) ? Vector{T}(undef, b) :
        what == BASIN_HOPPING_RNG_STATES ? Vector{UInt64}(undef, b) :
        what == BASIN_HOPPING_REC_NORMALS ? Array{T}(undef, 3, n, cap, b) :
        what in (BASIN_HOPPING_REC_UNIFORM, BASIN_HOPPING_REC_TRIAL_ENERGY) ? Array{T}(undef, cap, b) :
        what == BASIN_HOPPING_REC_QUENCH_ITERATIONS ? Array{Int32}(undef, cap, b) :
        what == BASIN_HOPPING_REC_CODE ? Array{Int8}(undef, cap, b) : Vector{Int64}(undef, b)
    check(ccall((:dzo_basin_hopping_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), bh.handle, what, r))
    return r
end

"""`set_array!(bh, what, values)`: BASIN_HOPPING_RADII (a vector of T) or BASIN_HOPPING_RNG_STATES (of UInt64); blocks."""
function set_array!(bh::BasinHopping{T}, what::Integer, values::AbstractVector) where {T}
    v = what == BASIN_HOPPING_RNG_STATES ? Vector{UInt64}(values) : Vector{T}(values)
    @assert length(v) == bh.batch
    check(ccall((:dzo_basin_hopping_set, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), bh.handle, what, v))
    return bh
end

"""Device address of one of the BASIN_HOPPING_* arrays (no wait)."""
function array_pointer(bh::BasinHopping, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_basin_hopping_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), bh.handle, what, p))
    return p[]
end

################################################################################ batched eigenvector following
# (not exercised in the build container either; the Python class ModeFollowing binds the same entry points and IS tested)
#
# Eigenvector following (Cerjan-Miller / Wales; include/dzo.h states the step) of `batch` clusters at once: per step the dense
# Hessians, their eigenvalues and eigenvectors and the step kernel, with no host wait in between.  target_index 0 polishes
# minima, 1 searches transition states.  `points` is aliased and moved.

const MODEFOLLOW_ACTIVE, MODEFOLLOW_CONVERGED, MODEFOLLOW_FAILED = 0, 1, 2
# `what` of read_array (DZO_MODEFOLLOW_* of include/dzo.h)
const MODEFOLLOW_POINTS, MODEFOLLOW_GRADIENTS, MODEFOLLOW_ENERGIES, MODEFOLLOW_GRMS, MODEFOLLOW_STATUS, MODEFOLLOW_INDEX,
      MODEFOLLOW_ZEROS, MODEFOLLOW_FOLLOWED_MODE, MODEFOLLOW_STEP_LENGTHS, MODEFOLLOW_ITERATION_COUNTS, MODEFOLLOW_EIGENVALUES,
      MODEFOLLOW_EIGENVECTORS, MODEFOLLOW_SWEEPS, MODEFOLLOW_FOLLOW = 0:13

mutable struct ModeFollowing{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
end

"""`ModeFollowing(lj_energy, points, n_particles; target_index=0, max_step=0.2, zero_tol=1e-4, grad_tol=1e-10)`."""
function ModeFollowing(::typeof(lj_energy), points::HipVector{T}, n_particles::Integer; target_index::Integer=0, max_step::Real=0.2,
                       zero_tol::Real=1e-4, grad_tol::Real=1e-10, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_modefollow_batch_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, target_index, Float64(max_step), Float64(zero_tol),
                Float64(grad_tol), h))
    mf = ModeFollowing{T}(h[], points, n_particles, batch)
    finalizer(mf) do w
        w.handle != C_NULL && ccall((:dzo_modefollow_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return mf
end

"""The mode an instance without a followed vector starts on (0: the lowest non-zero mode)."""
set_start_mode!(mf::ModeFollowing, mode::Integer) =
    (check(ccall((:dzo_modefollow_batch_set_start_mode, libdzo), Cint, (Ptr{Cvoid}, Cint), mf.handle, mode)); mf)

"""An initial followed vector per instance: `directions` holds 3N elements per instance; copied."""
function set_directions!(mf::ModeFollowing{T}, directions::HipVector{T}) where {T}
    check(ccall((:dzo_modefollow_batch_set_directions, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), mf.handle, directions.ptr))
    synchronize()
    return mf
end

"""`step!(mf, steps; wait=true)`: `steps` steps of every ACTIVE instance.  Returns whether no instance is ACTIVE any more
(`wait=true`, blocking) or `nothing` (enqueued only)."""
function step!(mf::ModeFollowing, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_modefollow_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), mf.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_modefollow_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), mf.handle, steps, flag))
    return flag[] != 0
end

function count_active(mf::ModeFollowing)
    n = Ref{Int64}(0)
    check(ccall((:dzo_modefollow_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), mf.handle, n))
    return Int(n[])
end

"""`read_array(mf, what)`: a blocking host copy of one of the MODEFOLLOW_* arrays, in its own element type; vectors and
eigenvector matrices come back with the instance as the last dimension."""
function read_array(mf::ModeFollowing{T}, what::Integer) where {T}
    n, b = 3 * mf.n_particles, mf.batch
    r = what in (MODEFOLLOW_POINTS, MODEFOLLOW_GRADIENTS, MODEFOLLOW_EIGENVALUES, MODEFOLLOW_FOLLOW) ? Array{T}(undef, n, b) :
        what == MODEFOLLOW_EIGENVECTORS ? Array{T}(undef, n, n, b) :
        what == MODEFOLLOW_ENERGIES ? Vector{T}(undef, b) :
        what in (MODEFOLLOW_GRMS, MODEFOLLOW_STEP_LENGTHS) ? Vector{Float64}(undef, b) :
        what == MODEFOLLOW_ITERATION_COUNTS ? Vector{Int64}(undef, b) : Vector{Int32}(undef, b)
    check(ccall((:dzo_modefollow_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), mf.handle, what, r))
    return r
end

"""Device address of one of the MODEFOLLOW_* arrays (no wait)."""
function array_pointer(mf::ModeFollowing, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_modefollow_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), mf.handle, what, p))
    return p[]
end

"""`modefollow_apply!(points, eigenvalues, eigenvectors, n_particles; ...)`: ONE step of every instance from modes the caller
supplies (`dzo_modefollow_batch_apply`); `points` is moved.  `target_index=1` needs `follow` (3N per instance) and `follow_set`
(a `HipVector{Float32}` of `batch` elements used as four bytes per instance: zero bits = not set).  Returns the status of every
instance as a `Vector{Int32}`.  Blocks."""
function modefollow_apply!(points::HipVector{T}, eigenvalues::HipVector{T}, eigenvectors::HipVector{T}, n_particles::Integer;
                           target_index::Integer=0, start_mode::Integer=0, max_step::Real=0.2, zero_tol::Real=1e-4, grad_tol::Real=0.0,
                           follow::Union{Nothing,HipVector{T}}=nothing, follow_set::Union{Nothing,HipVector{Float32}}=nothing, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    status = HipVector{Float32}(undef, batch)               # four bytes per instance: read back as Int32
    check(ccall((:dzo_modefollow_batch_apply, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cdouble, Cdouble, Cdouble,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, eigenvalues.ptr, eigenvectors.ptr,
                follow === nothing ? C_NULL : follow.ptr, follow_set === nothing ? C_NULL : follow_set.ptr, target_index, start_mode,
                Float64(max_step), Float64(zero_tol), Float64(grad_tol), C_NULL, C_NULL, C_NULL, C_NULL, status.ptr, C_NULL, C_NULL, C_NULL,
                C_NULL))
    return collect(reinterpret(Int32, Array(status)))
end

function run_steps!(mf::ModeFollowing, max_steps::Integer, steps_per_call::Integer=10)
    taken = 0
    done = count_active(mf) == 0
    while !done && taken < max_steps
        k = min(steps_per_call, max_steps - taken)
        done = step!(mf, k)
        taken += k
    end
    return mf
end

"""`polish_minima(lj_energy, points, n_particles; grad_tol=1e-10, max_steps=50, ...)`: target index 0 on the points a quench
left, in place, until `grms <= grad_tol`; returns the `ModeFollowing`."""
function polish_minima(f::typeof(lj_energy), points::HipVector{T}, n_particles::Integer; grad_tol::Real=1e-10, max_steps::Integer=50,
                       max_step::Real=0.2, zero_tol::Real=1e-4) where {T}
    return run_steps!(ModeFollowing(f, points, n_particles; target_index=0, max_step=max_step, zero_tol=zero_tol, grad_tol=grad_tol), max_steps)
end

"""`find_saddles(lj_energy, minima, n_particles; start_mode=0, kick=0.05, ...)`: polishes the minima, displaces each by `kick`
along its `start_mode`-th non-zero eigenvector, sets that eigenvector as the followed vector and follows it uphill (target index
1).  Returns `(saddles, polished)`, two `ModeFollowing`; `minima` ends holding the saddle searches' points."""
function find_saddles(f::typeof(lj_energy), minima::HipVector{T}, n_particles::Integer; start_mode::Integer=0, kick::Real=0.05,
                      grad_tol::Real=1e-10, max_steps::Integer=300, max_step::Real=0.1, zero_tol::Real=1e-4, polish_steps::Integer=50) where {T}
    polished = polish_minima(f, minima, n_particles; grad_tol=grad_tol, max_steps=polish_steps, zero_tol=zero_tol)
    lam, modes, x = read_array(polished, MODEFOLLOW_EIGENVALUES), read_array(polished, MODEFOLLOW_EIGENVECTORS), read_array(polished, MODEFOLLOW_POINTS)
    dirs = zeros(T, size(x))
    for b in 1:polished.batch
        nonzero = findall(v -> abs(v) > zero_tol, lam[:, b])
        length(nonzero) > start_mode && (dirs[:, b] = modes[:, nonzero[start_mode + 1], b])
    end
    kicked = HipVector(vec(x .+ T(kick) .* dirs))
    check(ccall((:dzo_memcpy_d2d, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), minima.ptr, kicked.ptr, sizeof(T) * length(minima)))
    saddles = ModeFollowing(f, minima, n_particles; target_index=1, max_step=max_step, zero_tol=zero_tol, grad_tol=grad_tol)
    set_start_mode!(saddles, start_mode)
    set_directions!(saddles, HipVector(vec(dirs)))
    return run_steps!(saddles, max_steps), polished
end

################################################################################ batched hybrid eigenvector following
# (not exercised in the build container either; the Python class HybridModeFollowing binds the same entry points and IS tested)
#
# Hybrid eigenvector following (Munro & Wales 1999; include/dzo.h states the step) of `batch` clusters of up to 1024 particles
# at once: per step the lowest mode is refined from the previous step's vector by a few Hessian-vector products, then the point
# steps uphill along it and relaxes orthogonally to it by a few gradient steps.  No dense Hessian.  `points` is aliased and moved.

const HYBRIDEF_ACTIVE, HYBRIDEF_CONVERGED, HYBRIDEF_FAILED = 0, 1, 2
# `what` of read_array (DZO_HYBRIDEF_* of include/dzo.h)
const HYBRIDEF_POINTS, HYBRIDEF_GRADIENTS, HYBRIDEF_ENERGIES, HYBRIDEF_GRMS, HYBRIDEF_STATUS, HYBRIDEF_EIGENVALUES, HYBRIDEF_MODES,
      HYBRIDEF_MODE_RESIDUALS, HYBRIDEF_PROJECTIONS, HYBRIDEF_UPHILL_STEPS, HYBRIDEF_TANGENT_STEPS, HYBRIDEF_ITERATION_COUNTS,
      HYBRIDEF_PRODUCTS, HYBRIDEF_EVALUATIONS = 0:13

mutable struct HybridModeFollowing{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
end

"""`HybridModeFollowing(lj_energy, points, n_particles; directions=nothing, max_step=0.1, tangent_steps=10, tangent_steps_convex=2,
tangent_cap=0.05, tangent_first=0.01, krylov=8, mode_cycles=1, mode_tol=1e-3, zero_tol=1e-4, grad_tol=1e-10, seed=0)`.
`directions`: the first modes, laid out like `points`, or `nothing` to draw them in the kernel from `seed`."""
function HybridModeFollowing(::typeof(lj_energy), points::HipVector{T}, n_particles::Integer; directions::Union{Nothing,HipVector{T}}=nothing,
                             max_step::Real=0.1, tangent_steps::Integer=10, tangent_steps_convex::Integer=2, tangent_cap::Real=0.05,
                             tangent_first::Real=0.01, krylov::Integer=8, mode_cycles::Integer=1, mode_tol::Real=1e-3, zero_tol::Real=1e-4,
                             grad_tol::Real=1e-10, seed::Integer=0, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_hybridef_batch_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Cint, Cdouble, Cdouble, Cint, Cint, Cdouble, Cdouble, Cdouble,
                 UInt64, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, directions === nothing ? C_NULL : directions.ptr,
                Float64(max_step), tangent_steps, tangent_steps_convex, Float64(tangent_cap), Float64(tangent_first), krylov, mode_cycles,
                Float64(mode_tol), Float64(zero_tol), Float64(grad_tol), UInt64(seed), h))
    hf = HybridModeFollowing{T}(h[], points, n_particles, batch)
    finalizer(hf) do w
        w.handle != C_NULL && ccall((:dzo_hybridef_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return hf
end

"""The mode the next refinement of every instance starts from: `directions` holds 3N elements per instance; copied."""
function set_directions!(hf::HybridModeFollowing{T}, directions::HipVector{T}) where {T}
    check(ccall((:dzo_hybridef_batch_set_directions, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), hf.handle, directions.ptr))
    synchronize()
    return hf
end

"""`step!(hf, steps; wait=true)`: `steps` steps of every ACTIVE instance.  Returns whether no instance is ACTIVE any more
(`wait=true`, blocking) or `nothing` (enqueued only)."""
function step!(hf::HybridModeFollowing, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_hybridef_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), hf.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_hybridef_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), hf.handle, steps, flag))
    return flag[] != 0
end

function count_active(hf::HybridModeFollowing)
    n = Ref{Int64}(0)
    check(ccall((:dzo_hybridef_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), hf.handle, n))
    return Int(n[])
end

"""`read_array(hf, what)`: a blocking host copy of one of the HYBRIDEF_* arrays, in its own element type; vectors come back with
the instance as the last dimension."""
function read_array(hf::HybridModeFollowing{T}, what::Integer) where {T}
    n, b = 3 * hf.n_particles, hf.batch
    r = what in (HYBRIDEF_POINTS, HYBRIDEF_GRADIENTS, HYBRIDEF_MODES) ? Array{T}(undef, n, b) :
        what in (HYBRIDEF_ENERGIES, HYBRIDEF_EIGENVALUES, HYBRIDEF_PROJECTIONS, HYBRIDEF_UPHILL_STEPS) ? Vector{T}(undef, b) :
        what in (HYBRIDEF_GRMS, HYBRIDEF_MODE_RESIDUALS) ? Vector{Float64}(undef, b) :
        what in (HYBRIDEF_ITERATION_COUNTS, HYBRIDEF_PRODUCTS, HYBRIDEF_EVALUATIONS) ? Vector{Int64}(undef, b) : Vector{Int32}(undef, b)
    check(ccall((:dzo_hybridef_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), hf.handle, what, r))
    return r
end

"""Device address of one of the HYBRIDEF_* arrays (no wait)."""
function array_pointer(hf::HybridModeFollowing, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_hybridef_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), hf.handle, what, p))
    return p[]
end

"""`hybridef_apply!(points, eigenvalues, modes, n_particles; ...)`: ONE step of every instance from a mode the caller supplies
(`dzo_hybridef_batch_apply`): `eigenvalues` holds one value and `modes` a unit vector of 3N elements per instance; `points` is
moved.  Returns the status of every instance as a `Vector{Int32}`.  Blocks."""
function hybridef_apply!(points::HipVector{T}, eigenvalues::HipVector{T}, modes::HipVector{T}, n_particles::Integer; max_step::Real=0.1,
                         tangent_steps::Integer=10, tangent_steps_convex::Integer=2, tangent_cap::Real=0.05, tangent_first::Real=0.01,
                         zero_tol::Real=1e-4, grad_tol::Real=0.0, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    status = HipVector{Float32}(undef, batch)               # four bytes per instance: read back as Int32
    check(ccall((:dzo_hybridef_batch_apply, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, eigenvalues.ptr, modes.ptr, Float64(max_step),
                tangent_steps, tangent_steps_convex, Float64(tangent_cap), Float64(tangent_first), Float64(zero_tol), Float64(grad_tol),
                C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, status.ptr, C_NULL))
    return collect(reinterpret(Int32, Array(status)))
end

function run_steps!(hf::HybridModeFollowing, max_steps::Integer, steps_per_call::Integer=20)
    taken = 0
    done = count_active(hf) == 0
    while !done && taken < max_steps
        k = min(steps_per_call, max_steps - taken)
        done = step!(hf, k)
        taken += k
    end
    return hf
end

"""`find_saddles_hybrid(lj_energy, minima, n_particles; kick=0.05, ...)`: takes the lowest mode of every minimum (`lowest_modes`
to the loose relative residual `start_res_tol`), displaces every point by `kick` along its vector, sets that vector as the first
mode and runs a `HybridModeFollowing` for at most `max_steps` steps.  Returns it; `minima` ends holding the searches' points."""
function find_saddles_hybrid(f::typeof(lj_energy), minima::HipVector{T}, n_particles::Integer; kick::Real=0.05, grad_tol::Real=1e-10,
                             max_steps::Integer=300, max_step::Real=0.1, zero_tol::Real=1e-4, start_res_tol::Real=1e-6, seed::Integer=0,
                             options...) where {T}
    vectors = lowest_modes(minima, n_particles; res_tol=start_res_tol, seed=seed)[2]
    axpy!(kick, vectors, minima)
    search = HybridModeFollowing(f, minima, n_particles; directions=vectors, max_step=max_step, zero_tol=zero_tol, grad_tol=grad_tol, seed=seed,
                                 options...)
    return run_steps!(search, max_steps)
end

"""`quench(lj_energy, points, n_particles; ...)`: run the batched optimizer on `points` (in place) until every instance is
stuck or `max_steps`; returns the optimizer."""
function quench(f::typeof(lj_energy), points::HipVector{T}, n_particles::Integer; history_length::Integer=10,
                initial_step_length::Real=0.01, steps_per_launch::Integer=50, max_steps::Integer=2000) where {T}
    opt = BatchedLBFGSOptimizer(f, points, n_particles, initial_step_length, history_length)
    taken = 0
    done = count_active(opt) == 0
    while !done && taken < max_steps
        k = min(steps_per_launch, max_steps - taken)
        done = step!(opt, k)
        taken += k
    end
    return opt
end

################################################################################ structure fingerprints, classification, pathways
# (not exercised in the build container either; the Python functions of the same names bind the same entry points and ARE tested)

"""`structure_fingerprints(points, n_particles)`: the fingerprint of every instance in one launch (include/dzo.h, "Structure
fingerprints"): per-particle energies sorted ascending, then squared distances from the centroid sorted ascending.  Unchanged
by rotation, translation, reflection and relabelling beyond rounding; blind to mirror images.  Returns
`(fingerprints::HipVector{T} (2N, batch), energies::Vector{T})`.  Blocks."""
function structure_fingerprints(points::HipVector{T}, n_particles::Integer; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch && batch >= 1
    fingerprints = HipVector{T}(undef, 2 * n_particles * batch)
    energies = HipVector{T}(undef, batch)
    check(ccall((:dzo_structure_batch_fingerprint, libdzo), Cint, (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, fingerprints.ptr, energies.ptr))
    return fingerprints, Array(energies)
end

"""`classify_structures(fingerprints, length, tol)`: greedy leader labels of the `length`-element vectors in `fingerprints` on
the device: a and b match iff `|a_i - b_i| <= tol * max(1, |a_i|, |b_i|)` for every i (fp64); instance k takes the label of the
first representative before it that it matches, or becomes one; a non-finite vector gets -1.  Returns `(labels::Vector{Int32}
(0-based, as the library numbers them), representatives::Vector{Int} (0-based))`.  Blocks."""
function classify_structures(fingerprints::HipVector{T}, length_::Integer, tol::Real) where {T}
    batch = div(length(fingerprints), length_)
    @assert length(fingerprints) == length_ * batch && batch >= 1
    labels_dev = HipVector{Float32}(undef, batch)            # four bytes per label: read back as Int32
    count = Ref{Cint}(0)
    check(ccall((:dzo_structure_batch_classify, libdzo), Cint, (Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}, Ref{Cint}),
                length_, batch, dtype_code(T), fingerprints.ptr, Float64(tol), labels_dev.ptr, count))
    labels = collect(reinterpret(Int32, Array(labels_dev)))
    representatives = [k - 1 for k in 1:batch if labels[k] == k - 1]
    @assert length(representatives) == count[]
    return labels, representatives
end

"""`connect_saddles(lj_energy, saddles, modes, n_particles; displacement, tol, known_minima=nothing, ...)`: which two minima every
transition state joins.  The 2 batch points `saddle +- displacement * mode` are formed on the device, quenched together by
`BatchedLBFGSOptimizer`s (restarted until no point moves), and `[known_minima | ends]` is fingerprinted and classified with `tol`.  `displacement` and `tol` have no
default (README.md, the structure block, has measured guidance).  Returns a named tuple `(minima, minimum_energies,
saddle_energies, edges, barriers, degenerate)`; `edges` is `batch x 2`, 1-based indices into the columns of `minima`, 0 where an
end was not stuck and at rest after `max_steps` or has a non-finite fingerprint."""
function connect_saddles(f::typeof(lj_energy), saddles::HipVector{T}, modes::HipVector{T}, n_particles::Integer; displacement::Real, tol::Real,
                         known_minima::Union{Nothing,HipVector{T}}=nothing, history_length::Integer=10, initial_step_length::Real=0.01,
                         steps_per_launch::Integer=50, max_steps::Integer=2000) where {T}
    n3 = 3 * n_particles
    batch = div(length(saddles), n3)
    @assert length(saddles) == n3 * batch && length(modes) == length(saddles)
    known = known_minima === nothing ? 0 : div(length(known_minima), n3)
    both = HipVector{T}(undef, (known + 2 * batch) * n3)
    part(offset, count) = HipVector{T}(both.ptr + offset * n3 * sizeof(T), count * n3)
    known > 0 && copy!(part(0, known), known_minima)
    for (side, sign) in enumerate((1.0, -1.0))
        end_ = part(known + (side - 1) * batch, batch)
        copy!(end_, saddles)
        axpy!(sign * displacement, modes, end_)
    end
    # "stuck" alone does not say "at rest": next to a saddle the first pair has s.y < 0, the L-BFGS direction points uphill and
    # the search halves the step to nothing on a slope.  A fresh optimizer (empty history) takes over until one leaves every
    # energy as it was, to the bit.
    stuck = falses(2 * batch)
    before = nothing
    taken = 0
    while taken < max_steps && !all(stuck)
        budget = max_steps - taken
        opt = quench(f, part(known, 2 * batch), n_particles; history_length=history_length, initial_step_length=initial_step_length,
                     steps_per_launch=steps_per_launch, max_steps=budget)
        taken += max(steps_per_launch, Int(maximum(iteration_counts(opt))))
        now = objective_values(opt)
        before === nothing || (stuck = stuck_flags(opt) .& (reinterpret.(UInt64, Float64.(now)) .== reinterpret.(UInt64, Float64.(before))))
        before = now
        finalize(opt)
    end
    fingerprints, energies = structure_fingerprints(both, n_particles)
    for k in findall(.!stuck)                                # an end that is still moving names no minimum
        fill!(HipVector{T}(fingerprints.ptr + (known + k - 1) * 2 * n_particles * sizeof(T), 1), NaN)
    end
    labels, representatives = classify_structures(fingerprints, 2 * n_particles, tol)
    position = Dict(r => i for (i, r) in enumerate(representatives))
    minima = HipVector{T}(undef, n3 * length(representatives))
    for (i, r) in enumerate(representatives)
        copy!(HipVector{T}(minima.ptr + (i - 1) * n3 * sizeof(T), n3), part(r, 1))
    end
    minimum_energies = energies[representatives .+ 1]
    saddle_energies = Array(pairwise_batch_energy_gradient!(HipVector{T}(undef, batch), HipVector{T}(undef, n3 * batch), saddles, n_particles))
    edges = [get(position, Int(labels[known + (side - 1) * batch + b]), 0) for b in 1:batch, side in 1:2]
    barriers = [edges[b, side] > 0 ? saddle_energies[b] - minimum_energies[edges[b, side]] : T(NaN) for b in 1:batch, side in 1:2]
    degenerate = [edges[b, 1] > 0 && edges[b, 1] == edges[b, 2] for b in 1:batch]
    return (minima=minima, minimum_energies=minimum_energies, saddle_energies=saddle_energies, edges=edges, barriers=barriers,
            degenerate=degenerate, both=both)
end

################################################################################ batched nudged elastic band
# (not exercised in the build container either; the Python class ElasticBand binds the same entry points and IS tested)
#
# The nudged elastic band with a climbing image (Henkelman & Jonsson 2000; include/dzo.h states the iteration) of `batch` pairs of
# minima at once: `band` holds n_images images of n_particles particles per band, image m of band b at 3 n_particles (n_images b + m),
# aliased and moved; images 0 and n_images - 1 are the fixed ends.

const NEB_MAX_PARTICLES, NEB_MAX_IMAGES = 1024, 32
const NEB_ACTIVE, NEB_CONVERGED, NEB_FAILED = 0, 1, 2
const NEB_SHAPE_WAVE, NEB_SHAPE_BLOCK = 0, 1
const NEB_STORAGE_LDS, NEB_STORAGE_MEMORY = 0, 1
# `what` of read_array (DZO_NEB_* of include/dzo.h)
const NEB_BAND, NEB_VELOCITIES, NEB_FORCES, NEB_TANGENTS, NEB_ENERGIES, NEB_FORCE_RMS, NEB_RESIDUALS, NEB_CLIMBING_IMAGES,
      NEB_HIGHEST_IMAGES, NEB_STATUS, NEB_ITERATION_COUNTS = 0:10

mutable struct ElasticBand{T}
    handle::Ptr{Cvoid}
    band::HipVector{T}
    n_particles::Int
    n_images::Int
    batch::Int
end

"""`neb_plan(T, n_particles, n_images)`: `(shape, storage, lds_bytes)` of `dzo_neb_plan`; a pure function, needs no device."""
function neb_plan(::Type{T}, n_particles::Integer, n_images::Integer) where {T}
    shape, storage, lds = Ref{Cint}(0), Ref{Cint}(0), Ref{Int64}(0)
    check(ccall((:dzo_neb_plan, libdzo), Cint, (Int64, Cint, Cint, Ref{Cint}, Ref{Cint}, Ref{Int64}),
                n_particles, n_images, dtype_code(T), shape, storage, lds))
    return Int(shape[]), Int(storage[]), Int(lds[])
end

"""`interpolate_band!(band, a, b, n_particles, n_images)`: the straight bands between the points `a` and `b` (3N elements per
band, in a common frame): images 0 and n_images - 1 are copies of `a` and `b`.  Returns `band`."""
function interpolate_band!(band::HipVector{T}, a::HipVector{T}, b::HipVector{T}, n_particles::Integer, n_images::Integer) where {T}
    ensure_init()
    batch = div(length(a), 3 * n_particles)
    @assert length(a) == 3 * n_particles * batch && length(b) == length(a) && length(band) == length(a) * n_images
    check(ccall((:dzo_neb_batch_interpolate, libdzo), Cint, (Int64, Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                n_particles, n_images, batch, dtype_code(T), a.ptr, b.ptr, band.ptr))
    return band
end

"""`ElasticBand(lj_energy, band, n_particles, n_images; force_tol, spring=1.0, dt=0.02, max_move=0.1, climb=true, climb_after=50)`.
`force_tol` has no default: what a band can reach depends on the element type."""
function ElasticBand(::typeof(lj_energy), band::HipVector{T}, n_particles::Integer, n_images::Integer; force_tol::Real, spring::Real=1.0,
                     dt::Real=0.02, max_move::Real=0.1, climb::Bool=true, climb_after::Integer=50, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = div(length(band), 3 * n_particles * n_images)
    @assert length(band) == 3 * n_particles * n_images * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_neb_batch_create, libdzo), Cint,
                (Cint, Int64, Cint, Int64, Cint, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cdouble, Cint, Int64, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, n_images, batch, dtype_code(T), band.ptr, Float64(spring), Float64(dt), Float64(max_move),
                Float64(force_tol), climb ? 1 : 0, climb_after, h))
    eb = ElasticBand{T}(h[], band, n_particles, n_images, batch)
    finalizer(eb) do w
        w.handle != C_NULL && ccall((:dzo_neb_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return eb
end

"""`step!(eb, steps; wait=true)`: ONE launch that iterates every ACTIVE band `steps` times.  Returns whether no band is ACTIVE any
more (`wait=true`, blocking) or `nothing` (enqueued only)."""
function step!(eb::ElasticBand, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_neb_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), eb.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_neb_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), eb.handle, steps, flag))
    return flag[] != 0
end

function count_active(eb::ElasticBand)
    n = Ref{Int64}(0)
    check(ccall((:dzo_neb_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), eb.handle, n))
    return Int(n[])
end

"""`read_array(eb, what)`: a blocking host copy of one of the NEB_* arrays, in its own element type; the band is the last
dimension, the image the one before it."""
function read_array(eb::ElasticBand{T}, what::Integer) where {T}
    n, m, b = 3 * eb.n_particles, eb.n_images, eb.batch
    r = what in (NEB_BAND, NEB_VELOCITIES, NEB_FORCES, NEB_TANGENTS) ? Array{T}(undef, n, m, b) :
        what == NEB_ENERGIES ? Array{T}(undef, m, b) : what == NEB_FORCE_RMS ? Array{Float64}(undef, m, b) :
        what == NEB_RESIDUALS ? Vector{Float64}(undef, b) : what == NEB_ITERATION_COUNTS ? Vector{Int64}(undef, b) : Vector{Int32}(undef, b)
    check(ccall((:dzo_neb_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), eb.handle, what, r))
    return r
end

"""Device address of one of the NEB_* arrays (no wait)."""
function array_pointer(eb::ElasticBand, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_neb_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), eb.handle, what, p))
    return p[]
end

"""`neb_apply!(band, velocities, n_particles, n_images; ...)`: ONE iteration of every band from the band and the velocities
given (`dzo_neb_batch_apply`), both moved.  Returns the status of every band as a `Vector{Int32}`; the other records of the
entry point (energies, gradients, forces, tangents, ...) are not asked for here: an `ElasticBand` stepped once has them.  Blocks."""
function neb_apply!(band::HipVector{T}, velocities::HipVector{T}, n_particles::Integer, n_images::Integer; spring::Real=1.0, dt::Real=0.02,
                    max_move::Real=0.1, force_tol::Real=0.0, climb::Bool=true, radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    batch = div(length(band), 3 * n_particles * n_images)
    @assert length(band) == 3 * n_particles * n_images * batch && length(velocities) == length(band)
    # HipVector holds the two floating-point types only: four bytes per band, written as int32 by the kernel and read back as such
    status = HipVector{Float32}(undef, batch)
    check(ccall((:dzo_neb_batch_apply, libdzo), Cint,
                (Cint, Int64, Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cdouble, Cint,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                Cint(radial), n_particles, n_images, batch, dtype_code(T), band.ptr, velocities.ptr, Float64(spring), Float64(dt),
                Float64(max_move), Float64(force_tol), climb ? 1 : 0,
                C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, status.ptr))
    return collect(reinterpret(Int32, Array(status)))
end

"""Destroys the handle now (the finalizer would otherwise, at some later collection); the band stays the caller's."""
function destroy!(eb::ElasticBand)
    eb.handle != C_NULL && ccall((:dzo_neb_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), eb.handle)
    eb.handle = C_NULL
    return nothing
end

function run_steps!(eb::ElasticBand, max_iterations::Integer, steps_per_call::Integer=100)
    taken = 0
    done = count_active(eb) == 0
    while !done && taken < max_iterations
        k = min(steps_per_call, max_iterations - taken)
        done = step!(eb, k)
        taken += k
    end
    return eb
end

################################################################################ rigid and permutational alignment of pairs
# (not exercised in the build container either; the Python functions of the same names bind the same entry points and ARE tested)
const ALIGN_MAX_PARTICLES, ALIGN_MAX_RANDOM_TRIALS, ALIGN_MAX_CYCLES = 1024, 64, 64
const ALIGN_TRIAL_IDENTITY, ALIGN_TRIAL_PRINCIPAL = 1, 2
const ALIGN_CONVERGED, ALIGN_CYCLE_LIMIT, ALIGN_FAILED = 0, 1, 2

# int32 results come back through four-byte device vectors (the method of classify_structures)
int32_array(v::HipVector{Float32}) = collect(reinterpret(Int32, Array(v)))

"""`assign_particles(a, b, n_particles)`: for every pair of points (3N elements each, `[x | y | z]`; neither is changed) the
permutation p that minimises `sum_i |a_i - b_p(i)|^2` in the frames given, by the shortest augmenting path in fp64 on the device
(`dzo_align_batch_assign`).  Returns `(perm::Matrix{Int32} (N x batch, 0-based as the library numbers them), cost::Vector{Float64})`.
Blocks."""
function assign_particles(a::HipVector{T}, b::HipVector{T}, n_particles::Integer) where {T}
    batch = div(length(a), 3 * n_particles)
    @assert length(a) == 3 * n_particles * batch && length(b) == length(a) && batch >= 1
    perm = HipVector{Float32}(undef, n_particles * batch)
    cost = HipVector{Float64}(undef, batch)
    check(ccall((:dzo_align_batch_assign, libdzo), Cint, (Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                n_particles, batch, dtype_code(T), a.ptr, b.ptr, perm.ptr, cost.ptr))
    return reshape(int32_array(perm), Int(n_particles), batch), Array(cost)
end

"""`align_pairs(a, b, n_particles; trials=ALIGN_TRIAL_IDENTITY | ALIGN_TRIAL_PRINCIPAL, random_trials=8, max_cycles=20,
allow_inversion=false, seed=0, want_trials=false)`: brings every `b[k]` onto `a[k]` by a translation, a rotation, a relabelling of
its identical particles and, with `allow_inversion`, an inversion (`dzo_align_batch_pairs`; include/dzo.h states the rule).
Returns a named tuple: `aligned` (a HipVector, 3N per pair: b in a's frame with a's labels), `permutations` (N x batch, 0-based),
`rotations` (9 x batch, row-major, the inversion folded in), `distances`, `best_trials`, `cycles`, `status`, and
`trial_distances` (n_starts x batch, or `nothing`).  Blocks."""
function align_pairs(a::HipVector{T}, b::HipVector{T}, n_particles::Integer; trials::Integer=ALIGN_TRIAL_IDENTITY | ALIGN_TRIAL_PRINCIPAL,
                     random_trials::Integer=8, max_cycles::Integer=20, allow_inversion::Bool=false, seed::Integer=0,
                     want_trials::Bool=false) where {T}
    batch = div(length(a), 3 * n_particles)
    @assert length(a) == 3 * n_particles * batch && length(b) == length(a) && batch >= 1
    n_orient = (trials & 1) + 4 * ((trials >> 1) & 1) + random_trials
    n_starts = (allow_inversion ? 2 : 1) * n_orient
    aligned = HipVector{T}(undef, 3 * n_particles * batch)
    perm = HipVector{Float32}(undef, n_particles * batch)
    rotation, distance = HipVector{Float64}(undef, 9 * batch), HipVector{Float64}(undef, batch)
    best, cycles, status = HipVector{Float32}(undef, batch), HipVector{Float32}(undef, batch), HipVector{Float32}(undef, batch)
    per_trial = want_trials ? HipVector{Float64}(undef, max(n_starts, 1) * batch) : nothing
    check(ccall((:dzo_align_batch_pairs, libdzo), Cint,
                (Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                n_particles, batch, dtype_code(T), a.ptr, b.ptr, trials, random_trials, max_cycles, allow_inversion ? 1 : 0,
                seed % UInt64, aligned.ptr, perm.ptr, rotation.ptr, distance.ptr, best.ptr, cycles.ptr, status.ptr,
                want_trials ? per_trial.ptr : C_NULL))
    return (aligned=aligned, permutations=reshape(int32_array(perm), Int(n_particles), batch), rotations=reshape(Array(rotation), 9, batch),
            distances=Array(distance), best_trials=int32_array(best), cycles=int32_array(cycles), status=int32_array(status),
            trial_distances=want_trials ? reshape(Array(per_trial), max(n_starts, 1), batch) : nothing)
end

"""`connect_minima(lj_energy, a, b, n_particles, n_images; force_tol, grad_tol=1e-10, max_iterations=10000, refine_steps=100, ...)`:
interpolates between the minima `a` and `b` (3N elements per pair, in a common frame; neither is changed), relaxes the bands to
`force_tol`, and refines the climbing image of every CONVERGED band along its tangent with a `HybridModeFollowing`.
`align=true`, or a named tuple of `align_pairs` options, brings arbitrary pairs into a common frame first (`b` is replaced by the
aligned copy, and the result carries `alignment`; it is `nothing` otherwise).  Returns a
named tuple: `band`, `energies` (n_images x batch), `status`, `climbing_images`, `converged` (the indices of the CONVERGED bands),
`saddles` (3N per converged band), `saddle_energies`, `saddle_status`, `barriers` (batch x 2: from image 1 and from image n_images,
NaN for a band that did not converge)."""
function connect_minima(f::typeof(lj_energy), a::HipVector{T}, b::HipVector{T}, n_particles::Integer, n_images::Integer; force_tol::Real,
                        grad_tol::Real=1e-10, max_iterations::Integer=10000, steps_per_call::Integer=100, refine_steps::Integer=100,
                        align=false, options...) where {T}
    n3 = 3 * n_particles
    batch = div(length(a), n3)
    alignment = align === false ? nothing : align_pairs(a, b, n_particles; (align === true ? NamedTuple() : align)...)
    alignment === nothing || (b = alignment.aligned)
    band = interpolate_band!(HipVector{T}(undef, n3 * n_images * batch), a, b, n_particles, n_images)
    eb = run_steps!(ElasticBand(f, band, n_particles, n_images; force_tol=force_tol, options...), max_iterations, steps_per_call)
    energies, status, climbing = read_array(eb, NEB_ENERGIES), read_array(eb, NEB_STATUS), read_array(eb, NEB_CLIMBING_IMAGES)
    converged = [k for k in 1:batch if status[k] == NEB_CONVERGED && climbing[k] >= 0]
    saddles, tangents = HipVector{T}(undef, n3 * max(length(converged), 1)), HipVector{T}(undef, n3 * max(length(converged), 1))
    GC.@preserve eb begin                                   # the tangents are the handle's: it must outlive the copies
        tangent_ptr = array_pointer(eb, NEB_TANGENTS)
        for (i, k) in enumerate(converged)
            offset = ((k - 1) * n_images + Int(climbing[k])) * n3 * sizeof(T)
            copy!(HipVector{T}(saddles.ptr + (i - 1) * n3 * sizeof(T), n3), HipVector{T}(band.ptr + offset, n3))
            copy!(HipVector{T}(tangents.ptr + (i - 1) * n3 * sizeof(T), n3), HipVector{T}(tangent_ptr + offset, n3))
        end
        synchronize()
    end
    destroy!(eb)
    barriers = fill(T(NaN), batch, 2)
    saddle_energies, saddle_status = T[], Int32[]
    if !isempty(converged)
        search = run_steps!(HybridModeFollowing(f, saddles, n_particles; directions=tangents, grad_tol=grad_tol), refine_steps)
        saddle_energies, saddle_status = read_array(search, HYBRIDEF_ENERGIES), read_array(search, HYBRIDEF_STATUS)
        finalize(search)                                    # destroys the handle now; `saddles` stays
        for (i, k) in enumerate(converged)
            barriers[k, 1] = saddle_energies[i] - energies[1, k]
            barriers[k, 2] = saddle_energies[i] - energies[n_images, k]
        end
    end
    return (band=band, energies=energies, status=status, climbing_images=climbing, converged=converged, saddles=saddles,
            saddle_energies=saddle_energies, saddle_status=saddle_status, barriers=barriers, alignment=alignment)
end

################################################################################ transition-state candidates of many bands
# (not exercised in the build container either; the Python function of the same name binds the same entry point and IS tested.
# The connect cycle built on it, connect_pathways with its PathwayGraph, is Python only.)
const PATHWAY_MAX_PARTICLES, PATHWAY_MAX_IMAGES, PATHWAY_MAX_BATCH = 1024, 32, 1048576
const PATHWAY_OVERFLOW = 7

"""`band_candidates(band, energies, n_particles, n_images)`: the transition-state candidates of every band of `band` (3N n_images
elements per band, the layout of `ElasticBand`; not changed) from its energy profile `energies` (n_images per band, for instance
`array_pointer(eb, NEB_ENERGIES)` wrapped, or `pairwise_batch_energy_gradient!` of the band taken as points):
`dzo_pathway_batch_candidates`, include/dzo.h states the rule.  Interior image m is a candidate iff `E[m] > E[m-1]` and
`E[m] >= E[m+1]`.  Returns a named tuple, compacted band-major: `count`, `points` and `tangents` (HipVectors with room for the
most the bands can hold; the first `3N count` elements are the candidates), `energies`, `band_index` and `image_index` (0-based,
`count` each) and `offsets` (batch + 1).  Blocks."""
function band_candidates(band::HipVector{T}, energies::HipVector{T}, n_particles::Integer, n_images::Integer) where {T}
    n3 = 3 * n_particles
    batch = div(length(band), n3 * n_images)
    @assert length(band) == n3 * n_images * batch && length(energies) == n_images * batch && batch >= 1
    capacity = batch * div(n_images - 1, 2)
    points, tangents = HipVector{T}(undef, n3 * capacity), HipVector{T}(undef, n3 * capacity)
    cand_energies = HipVector{T}(undef, capacity)
    band_index, image_index = HipVector{Float32}(undef, capacity), HipVector{Float32}(undef, capacity)
    offsets = HipVector{Float32}(undef, batch + 1)
    count = Ref{Int64}(0)
    check(ccall((:dzo_pathway_batch_candidates, libdzo), Cint,
                (Int64, Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                 Ptr{Int64}),
                n_particles, n_images, batch, dtype_code(T), band.ptr, energies.ptr, capacity, points.ptr, tangents.ptr, cand_energies.ptr,
                band_index.ptr, image_index.ptr, offsets.ptr, count))
    k = Int(count[])
    return (count=k, points=points, tangents=tangents, energies=Array(cand_energies)[1:k], band_index=int32_array(band_index)[1:k],
            image_index=int32_array(image_index)[1:k], offsets=int32_array(offsets))
end

################################################################################ batched AdGD over Lennard-Jones clusters
# (not exercised in the build container either; the Python class BatchedAdGD binds the same entry points and IS tested)
#
# The live AdGDOptimizer (src/DZOptimization.jl:179-312, constraint_function! = nothing) of `batch` clusters at once, the
# sibling of BatchedLBFGSOptimizer without a history: the same layout of `points`, aliased (:238).

mutable struct BatchedAdGDOptimizer{T}
    handle::Ptr{Cvoid}
    points::HipVector{T}
    n_particles::Int
    batch::Int
end

"""`BatchedAdGDOptimizer(lj_energy, points, n_particles, initial_step_length)` (:245-271 per instance)."""
function BatchedAdGDOptimizer(::typeof(lj_energy), points::HipVector{T}, n_particles::Integer, initial_step_length::Real; radial::Integer=DZO_RADIAL_LENNARD_JONES) where {T}
    ensure_init()
    batch = div(length(points), 3 * n_particles)
    @assert length(points) == 3 * n_particles * batch
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_adgd_batch_create, libdzo), Cint,
                (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                Cint(radial), n_particles, batch, dtype_code(T), points.ptr, Float64(initial_step_length), h))
    opt = BatchedAdGDOptimizer{T}(h[], points, n_particles, batch)
    finalizer(opt) do w
        w.handle != C_NULL && ccall((:dzo_adgd_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), w.handle)
        w.handle = C_NULL
    end
    return opt
end

"""`step!(opt, steps; wait=true)`: `steps` calls of step!() (:274-312) of every instance that is not stuck, one launch.
Returns whether every instance is stuck (`wait=true`, blocking) or `nothing` (enqueued only)."""
function step!(opt::BatchedAdGDOptimizer, steps::Integer=1; wait::Bool=true)
    if !wait
        check(ccall((:dzo_adgd_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), opt.handle, steps, C_NULL))
        return nothing
    end
    flag = Ref{Cint}(0)
    check(ccall((:dzo_adgd_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), opt.handle, steps, flag))
    return flag[] != 0
end

set_max_halvings!(opt::BatchedAdGDOptimizer, v::Integer) =
    (check(ccall((:dzo_adgd_batch_set_max_halvings, libdzo), Cint, (Ptr{Cvoid}, Int64), opt.handle, v)); opt)

function count_active(opt::BatchedAdGDOptimizer)
    n = Ref{Int64}(0)
    check(ccall((:dzo_adgd_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), opt.handle, n))
    return Int(n[])
end

"""One of the per-instance arrays of element type `E` (a DZO_ADGD_BATCH_* constant of include/dzo.h with `batch` elements); blocks."""
function read_per_instance(opt::BatchedAdGDOptimizer, what::Integer, ::Type{E}) where {E}
    r = Vector{E}(undef, opt.batch)
    check(ccall((:dzo_adgd_batch_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), opt.handle, what, r))
    return r
end

objective_values(opt::BatchedAdGDOptimizer{T}) where {T} = read_per_instance(opt, 4, T)     # DZO_ADGD_BATCH_OBJECTIVES
iteration_counts(opt::BatchedAdGDOptimizer) = read_per_instance(opt, 7, Int64)             # DZO_ADGD_BATCH_ITERATION_COUNTS
stuck_flags(opt::BatchedAdGDOptimizer) = read_per_instance(opt, 6, Int32) .!= 0            # DZO_ADGD_BATCH_IS_STUCK
current_step_sizes(opt::BatchedAdGDOptimizer{T}) where {T} = read_per_instance(opt, 8, T)   # DZO_ADGD_BATCH_CURRENT_STEP_SIZES

"""Device address of one of the DZO_ADGD_BATCH_* arrays of include/dzo.h (no wait)."""
function array_pointer(opt::BatchedAdGDOptimizer, what::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_adgd_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), opt.handle, what, p))
    return p[]
end

# decorators of legacy/DZOptimization.jl:219-296, applied on the device
"""`with_l2!(p, lambda)`: L2RegularizationWrapper + L2GradientWrapper (legacy :225-249)."""
with_l2!(p::BuiltinProblem, lambda::Real) = (check(ccall((:dzo_problem_set_l2, libdzo), Cint, (Ptr{Cvoid}, Cdouble), p.handle, lambda)); p)
"""`with_box_gradient!(p, lo, hi)`: UniformBoxGradientWrapper (legacy :275-296)."""
with_box_gradient!(p::BuiltinProblem, lo::Real, hi::Real) =
    (check(ccall((:dzo_problem_set_box_gradient, libdzo), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cdouble), p.handle, 1, lo, hi)); p)
"""`with_box_constraint!(p, lo, hi)`: UniformBoxConstraint (legacy :258-272) as constraint_function!."""
with_box_constraint!(p::BuiltinProblem, lo::Real, hi::Real) =
    (check(ccall((:dzo_problem_set_box_constraint, libdzo), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cdouble), p.handle, 1, lo, hi)); p)
"""`UniformBoxConstraint(lo, hi)(x)` on a device vector (legacy :264-272)."""
struct UniformBoxConstraint{T}; lower_bound::T; upper_bound::T; end
function (c::UniformBoxConstraint)(x::HipVector{T}) where {T}
    check(ccall((:dzo_box_clamp, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Cdouble, Cdouble), x.len, dtype_code(T), x.ptr, c.lower_bound, c.upper_bound))
    return true
end

################################################################################ callbacks

# C trampolines: ctx is a pointer to a Julia Ref holding (constraint!, objective, gradient!, T, n)
struct Callbacks{C,F,G,T}
    constraint!::C
    objective::F
    gradient!::G
    n::Int
end
function _c_constraint(ctx::Ptr{Cvoid}, x::Ptr{Cvoid})::Cint
    cb = unsafe_pointer_to_objref(ctx)[]
    return Cint(cb.constraint!(_view(cb, x)) ? 1 : 0)
end
function _c_objective(ctx::Ptr{Cvoid}, x::Ptr{Cvoid})::Cdouble
    cb = unsafe_pointer_to_objref(ctx)[]
    return Cdouble(cb.objective(_view(cb, x)))
end
function _c_gradient(ctx::Ptr{Cvoid}, g::Ptr{Cvoid}, x::Ptr{Cvoid})::Cvoid
    cb = unsafe_pointer_to_objref(ctx)[]
    cb.gradient!(_view(cb, g), _view(cb, x))
    return nothing
end
_view(cb::Callbacks{C,F,G,T}, p::Ptr{Cvoid}) where {C,F,G,T} = HipVector{T}(p, cb.n)

################################################################################ L-BFGS

abstract type AbstractOptimizer{T,A} end
function step! end

"""`LBFGSOptimizer(constraint!, objective, gradient!, x0, step, m)` (src/DZOptimization.jl:400-407)
or the full form with `f0, g0` (:347-356).  `objective` may be a `BuiltinProblem`, in which case
the whole step runs on the device.  Aliases `x0` as `current_point` (:393)."""
mutable struct LBFGSOptimizer{T,A,C,F,G} <: AbstractOptimizer{T,A}
    handle::Ptr{Cvoid}
    constraint_function!::C
    objective_function::F
    gradient_function!::G
    current_point::A
    history_length::Int
    keep::Any
    function LBFGSOptimizer{T,A,C,F,G}(h, c, f, g, x, m, keep) where {T,A,C,F,G}
        return finalizer(o -> ccall((:dzo_lbfgs_destroy, libdzo), Cint, (Ptr{Cvoid},), getfield(o, :handle)),
                         new{T,A,C,F,G}(h, c, f, g, x, m, keep))
    end
end

function LBFGSOptimizer(constraint!::C, objective::F, gradient!::G, x0::HipVector{T},
                        initial_step_length::Real, history_length::Int) where {T,C,F,G}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if objective isa BuiltinProblem && constraint! === nothing
        check(ccall((:dzo_lbfgs_create_problem, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                    objective.handle, history_length, x0.ptr, initial_step_length, h))
        return LBFGSOptimizer{T,HipVector{T},C,F,G}(h[], constraint!, objective, gradient!, x0, history_length, nothing)
    end
    cb = Ref(Callbacks{C,F,G,T}(constraint!, objective, gradient!, length(x0)))
    cf = constraint! === nothing ? C_NULL : @cfunction(_c_constraint, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
    check(ccall((:dzo_lbfgs_create_callbacks, libdzo), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                cf, @cfunction(_c_objective, Cdouble, (Ptr{Cvoid}, Ptr{Cvoid})),
                @cfunction(_c_gradient, Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})),
                pointer_from_objref(cb), length(x0), history_length, dtype_code(T), x0.ptr, initial_step_length, h))
    return LBFGSOptimizer{T,HipVector{T},C,F,G}(h[], constraint!, objective, gradient!, x0, history_length, cb)
end

function LBFGSOptimizer(constraint!::C, objective::F, gradient!::G, x0::HipVector{T}, f0::Real, g0::HipVector{T},
                        initial_step_length::Real, history_length::Int) where {T,C,F,G}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_lbfgs_create, libdzo), Cint, (Int64, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ref{Ptr{Cvoid}}),
                length(x0), history_length, dtype_code(T), x0.ptr, g0.ptr, f0, initial_step_length, h))
    cb = Ref(Callbacks{C,F,G,T}(constraint!, objective, gradient!, length(x0)))
    cf = constraint! === nothing ? C_NULL : @cfunction(_c_constraint, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
    check(ccall((:dzo_lbfgs_set_callbacks, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                h[], cf, @cfunction(_c_objective, Cdouble, (Ptr{Cvoid}, Ptr{Cvoid})),
                @cfunction(_c_gradient, Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), pointer_from_objref(cb)))
    return LBFGSOptimizer{T,HipVector{T},C,F,G}(h[], constraint!, objective, gradient!, x0, history_length, (cb, g0))
end

"""`step!(opt)` (src/DZOptimization.jl:454-509)."""
step!(opt::LBFGSOptimizer) = (check(ccall((:dzo_lbfgs_step, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)

"""`compute_lbfgs_step_direction!(opt)` (src/DZOptimization.jl:430-451): the two-loop recursion alone,
`opt.step_direction = -H_k * opt.current_gradient`."""
compute_lbfgs_step_direction!(opt::LBFGSOptimizer) =
    (check(ccall((:dzo_lbfgs_direction, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)

const BACKTRACKING, STRONG_WOLFE = Cint(0), Cint(1)

"""`set_safeguards!(opt; descent_check=false, steepest_descent_fallback=false)`: the legacy
optimizer's descent check (legacy/DZOptimization.jl:682-692) and steepest-descent fallback with
history reset (:588-610) as options of the live `step!`; both off = the reference."""
set_safeguards!(opt::LBFGSOptimizer; descent_check::Bool=false, steepest_descent_fallback::Bool=false) =
    (check(ccall((:dzo_lbfgs_set_safeguards, libdzo), Cint, (Ptr{Cvoid}, Cint, Cint), getfield(opt, :handle),
                 descent_check, steepest_descent_fallback)); opt)

"""`set_line_search!(opt, STRONG_WOLFE; c1=1e-4, c2=0.9, max_evals=40)`: strong-Wolfe search on the
`LineSearchEvaluator` quotients (src/DZOptimization.jl:84, :88-89); `BACKTRACKING` restores
`take_backtracking_step!` (:107-154)."""
set_line_search!(opt::LBFGSOptimizer, kind::Integer; c1::Real=0.0, c2::Real=0.0, max_evals::Integer=0) =
    (check(ccall((:dzo_lbfgs_set_line_search, libdzo), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cint),
                 getfield(opt, :handle), kind, c1, c2, max_evals)); opt)

_lb_i(o, w) = (v = Ref{Int64}(0); check(ccall((:dzo_lbfgs_get_i, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), getfield(o, :handle), w, v)); v[])
_lb_s(o, w) = (v = Ref{Cdouble}(0); check(ccall((:dzo_lbfgs_get_s, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), getfield(o, :handle), w, v)); v[])
function _lb_p(o::LBFGSOptimizer{T}, w, idx=0) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_lbfgs_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}), getfield(o, :handle), w, idx, p))
    return HipVector{T}(p[], length(getfield(o, :current_point)))
end
"""`read_field(opt, :current_point)` (also `:delta_point`, `:current_gradient`, `:delta_gradient`, `:step_direction`): the field as
a host `Vector{T}`, copied by the library itself (`dzo_lbfgs_read`).  No device pointer is handed out, so the step behind the read
does not have to check the aliased arrays for host writes (src/DZOptimization.jl:393; after `opt.current_point`, which hands the
pointer out, it does) -- the way to watch a run."""
function read_field(o::LBFGSOptimizer{T}, s::Symbol) where {T}
    w = findfirst(==(s), (:current_point, :delta_point, :current_gradient, :delta_gradient, :step_direction))
    w === nothing && throw(ArgumentError("read_field: unknown field $s"))
    out = Vector{T}(undef, length(getfield(o, :current_point)))
    check(ccall((:dzo_lbfgs_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}), getfield(o, :handle), w - 1, 0, out))
    return out
end
function _lb_hist(o::LBFGSOptimizer{T}, rho::Bool) where {T}   # (ccall needs a literal symbol name)
    buf = Vector{Cdouble}(undef, 64); cnt = Ref{Cint}(0)
    if rho
        check(ccall((:dzo_lbfgs_get_rho, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ref{Cint}), getfield(o, :handle), buf, 64, cnt))
    else
        check(ccall((:dzo_lbfgs_get_alpha, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ref{Cint}), getfield(o, :handle), buf, 64, cnt))
    end
    return T.(buf[1:cnt[]])
end

# Public fields of the reference (src/DZOptimization.jl:321-344); scalars come back boxed in
# 0-dim arrays like the reference's Array{T,0}, so `opt.is_stuck[]` reads the same.
function Base.getproperty(o::LBFGSOptimizer{T}, s::Symbol) where {T}
    s in (:is_stuck, :has_terminated, :has_converged) && return fill(_lb_i(o, 0) != 0)
    s === :iteration_count && return fill(Int(_lb_i(o, 1)))
    s === :current_objective_value && return fill(T(_lb_s(o, 0)))
    s === :delta_objective_value && return fill(T(_lb_s(o, 1)))
    s === :delta_point && return _lb_p(o, 1)
    s === :current_gradient && return _lb_p(o, 2)
    s === :delta_gradient && return _lb_p(o, 3)
    s === :step_direction && return _lb_p(o, 4)
    s === :delta_point_history && return [_lb_p(o, 5, i - 1) for i in 1:_lb_i(o, 4)]
    s === :delta_gradient_history && return [_lb_p(o, 6, i - 1) for i in 1:_lb_i(o, 4)]
    s === :rho_history && return _lb_hist(o, true)
    s === :alpha_history && return _lb_hist(o, false)
    s === :last_step_length && return fill(T(_lb_s(o, 2)))
    s === :history_resets && return Int(_lb_i(o, 8))
    s === :descent_resets && return Int(_lb_i(o, 9))
    # informational (include/dzo.h): steps taken as one sweep, their rejected first trials / second passes, and how the
    # history lives in HBM (0 slabs, 1 tiles of pairs, 2 tiles of points; tile arrangement 1 tile-major, 2 stream-major)
    s === :single_pass_steps && return Int(_lb_i(o, 11))
    s === :single_pass_rejections && return Int(_lb_i(o, 12))
    s === :single_pass_retries && return Int(_lb_i(o, 13))
    s === :ring_layout && return Int(_lb_i(o, 14))
    s === :tile_arrangement && return Int(_lb_i(o, 15))
    s === :pass_recomputes_gradients && return _lb_i(o, 16) != 0
    s === :pass_register_sets && return Int(_lb_i(o, 17))
    return getfield(o, s)
end

################################################################################ dense BFGS

"""`BFGSOptimizer(objective, gradient!, [constraint!,] x0, initial_step_length)` (README.md:33-36,
legacy/DZOptimization.jl:753-766).  Copies `x0` (:769)."""
mutable struct BFGSOptimizer{T,F,G,C}
    handle::Ptr{Cvoid}
    objective_function::F
    gradient_function!::G
    constraint_function!::C
    n::Int
    keep::Any
    function BFGSOptimizer{T,F,G,C}(h, f, g, c, n, keep) where {T,F,G,C}
        return finalizer(o -> ccall((:dzo_bfgs_destroy, libdzo), Cint, (Ptr{Cvoid},), getfield(o, :handle)),
                         new{T,F,G,C}(h, f, g, c, n, keep))
    end
end
BFGSOptimizer(objective, gradient!, x0::HipVector, step::Real) = BFGSOptimizer(objective, gradient!, nothing, x0, step)
# README.md:33-36 passes a host array (`rand(2)`): upload it (the optimizer copies x0 anyway, :769)
BFGSOptimizer(objective, gradient!, x0::Array{T}, step::Real) where {T<:Union{Float32,Float64}} =
    BFGSOptimizer(objective, gradient!, nothing, HipVector(x0), step)
BFGSOptimizer(objective, gradient!, constraint!, x0::Array{T}, step::Real) where {T<:Union{Float32,Float64}} =
    BFGSOptimizer(objective, gradient!, constraint!, HipVector(x0), step)
function BFGSOptimizer(objective::F, gradient!::G, constraint!::C, x0::HipVector{T}, step::Real) where {T,F,G,C}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if objective isa BuiltinProblem && constraint! === nothing
        check(ccall((:dzo_bfgs_create_problem, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}), objective.handle, x0.ptr, step, h))
        return BFGSOptimizer{T,F,G,C}(h[], objective, gradient!, constraint!, length(x0), nothing)
    end
    cb = Ref(Callbacks{C,F,G,T}(constraint!, objective, gradient!, length(x0)))
    cf = constraint! === nothing ? C_NULL : @cfunction(_c_constraint, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
    check(ccall((:dzo_bfgs_create_callbacks, libdzo), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                @cfunction(_c_objective, Cdouble, (Ptr{Cvoid}, Ptr{Cvoid})),
                @cfunction(_c_gradient, Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), cf,
                pointer_from_objref(cb), length(x0), dtype_code(T), x0.ptr, step, h))
    return BFGSOptimizer{T,F,G,C}(h[], objective, gradient!, constraint!, length(x0), cb)
end

"""`BFGSOptimizer(T, opt, objective_in_T)` (legacy/DZOptimization.jl:812-862): the same optimizer state in
another precision (fp32 warm start, fp64 finish); objective value, gradient and `H*g` are recomputed
in `T` (:825-836).  `objective_in_T` is the built-in problem of the target precision."""
function BFGSOptimizer(::Type{T}, opt::BFGSOptimizer, objective::BuiltinProblem{T}) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_bfgs_convert_problem, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                getfield(opt, :handle), objective.handle, h))
    return BFGSOptimizer{T,typeof(objective),Nothing,Nothing}(h[], objective, nothing, nothing, getfield(opt, :n), nothing)
end

"""`update_inverse_hessian!(H, step_length, d, delta_gradient, scratch)` (legacy/DZOptimization.jl:864-889) on
raw device arrays (`H` column-major n*n); rescales `d` in place (:874)."""
function update_inverse_hessian!(H::HipVector{T}, step_length::Real, d::HipVector{T}, delta_gradient::HipVector{T},
                                 scratch::HipVector{T}) where {T}
    check(ccall((:dzo_bfgs_update, libdzo), Cint,
                (Int64, Cint, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                length(d), dtype_code(T), H.ptr, step_length, d.ptr, delta_gradient.ptr, scratch.ptr, C_NULL, C_NULL))
    return H
end

"""`reset_inverse_hessian!(opt)`: `approximate_inverse_hessian = I`, `next_step_direction = gradient`
(the reset of legacy/DZOptimization.jl:981-986, `identity_matrix!` :712-720)."""
reset_inverse_hessian!(opt::BFGSOptimizer) = (check(ccall((:dzo_bfgs_reset, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)

"""`step!(opt)` (legacy/DZOptimization.jl:891-994)."""
step!(opt::BFGSOptimizer) = (check(ccall((:dzo_bfgs_step, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)

_bf_i(o, w) = (v = Ref{Int64}(0); check(ccall((:dzo_bfgs_get_i, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), getfield(o, :handle), w, v)); v[])
_bf_s(o, w) = (v = Ref{Cdouble}(0); check(ccall((:dzo_bfgs_get_s, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), getfield(o, :handle), w, v)); v[])
function _bf_p(o::BFGSOptimizer{T}, w, len=getfield(o, :n)) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_bfgs_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), getfield(o, :handle), w, p))
    return HipVector{T}(p[], len)
end
function Base.getproperty(o::BFGSOptimizer{T}, s::Symbol) where {T}
    s in (:has_converged, :has_terminated, :is_stuck) && return fill(_bf_i(o, 0) != 0)
    s === :iteration_count && return fill(Int(_bf_i(o, 1)))
    s === :last_step_type && return fill(Int(_bf_i(o, 3)))       # 0 Null, 1 GradientDescent, 2 BFGS (:727-731)
    s === :current_objective_value && return fill(T(_bf_s(o, 0)))
    s === :last_step_length && return fill(T(_bf_s(o, 1)))
    s === :current_point && return _bf_p(o, 0)
    s === :delta_point && return _bf_p(o, 1)
    s === :current_gradient && return _bf_p(o, 2)
    s === :delta_gradient && return _bf_p(o, 3)
    s === :next_step_direction && return _bf_p(o, 4)
    s === :approximate_inverse_hessian && return _bf_p(o, 5, getfield(o, :n)^2)   # column-major n*n
    return getfield(o, s)
end

"""`install_state!(opt; x, g, H, d, f, last_step_length, iteration_count, last_step_type, delta_point, delta_gradient)`:
overwrite the optimizer's state from host arrays ("save/load data in the middle of optimization",
README.md:11); `H` column-major n*n.  The device arrays are the state itself (`opt.current_point` etc. are
views of them); the host-side fields go through `dzo_bfgs_set_s / set_i`."""
function install_state!(opt::BFGSOptimizer{T}; x=nothing, g=nothing, H=nothing, d=nothing, f=nothing, last_step_length=nothing,
                        iteration_count=nothing, last_step_type=nothing, delta_point=nothing, delta_gradient=nothing) where {T}
    up(dst::HipVector, src) = (h = Array{T}(vec(src));
                               check(ccall((:dzo_memcpy_h2d, libdzo), Cint, (Ptr{Cvoid}, Ptr{T}, Int64), dst.ptr, h, sizeof(h))))
    x === nothing || up(opt.current_point, x)
    g === nothing || up(opt.current_gradient, g)
    H === nothing || up(opt.approximate_inverse_hessian, H)
    d === nothing || up(opt.next_step_direction, d)
    delta_point === nothing || up(opt.delta_point, delta_point)
    delta_gradient === nothing || up(opt.delta_gradient, delta_gradient)
    f === nothing || check(ccall((:dzo_bfgs_set_s, libdzo), Cint, (Ptr{Cvoid}, Cint, Cdouble), getfield(opt, :handle), 0, f))
    last_step_length === nothing || check(ccall((:dzo_bfgs_set_s, libdzo), Cint, (Ptr{Cvoid}, Cint, Cdouble), getfield(opt, :handle), 1, last_step_length))
    iteration_count === nothing || check(ccall((:dzo_bfgs_set_i, libdzo), Cint, (Ptr{Cvoid}, Cint, Int64), getfield(opt, :handle), 1, iteration_count))
    last_step_type === nothing || check(ccall((:dzo_bfgs_set_i, libdzo), Cint, (Ptr{Cvoid}, Cint, Int64), getfield(opt, :handle), 3, last_step_type))
    return opt
end

################################################################################ legacy gradient descent

"""`GradientDescentOptimizer(objective, gradient!, QuadraticLineSearch(), x0, step)`
(legacy/DZOptimization.jl:377-390); built-in objectives only in this thin binding.  The handle is a
BFGS-family handle, so the `BFGSOptimizer` getters apply (no `approximate_inverse_hessian`)."""
struct QuadraticLineSearch; max_increases::Int; end
QuadraticLineSearch() = QuadraticLineSearch(0)
function GradientDescentOptimizer(objective::BuiltinProblem{T}, ::Any, ls::QuadraticLineSearch, x0::HipVector{T}, step::Real) where {T}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_gd_create_problem, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}), objective.handle, x0.ptr, step, h))
    check(ccall((:dzo_bfgs_set_max_increases, libdzo), Cint, (Ptr{Cvoid}, Cint), h[], ls.max_increases))
    return GDHandle{T}(h[], length(x0), objective)
end
mutable struct GDHandle{T}
    handle::Ptr{Cvoid}
    n::Int
    keep::Any
    GDHandle{T}(h, n, keep) where {T} =
        finalizer(o -> ccall((:dzo_bfgs_destroy, libdzo), Cint, (Ptr{Cvoid},), getfield(o, :handle)), new{T}(h, n, keep))
end
step!(opt::GDHandle) = (check(ccall((:dzo_gd_step, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)
function Base.getproperty(o::GDHandle{T}, s::Symbol) where {T}      # the BFGS-family getters (include/dzo.h)
    s in (:has_terminated, :has_converged, :is_stuck) && return fill(_bf_i(o, 0) != 0)
    s === :iteration_count && return fill(Int(_bf_i(o, 1)))
    s === :current_objective_value && return fill(T(_bf_s(o, 0)))
    s === :last_step_length && return fill(T(_bf_s(o, 1)))
    if s in (:current_point, :delta_point, :current_gradient, :delta_gradient, :next_step_direction)
        w = findfirst(==(s), (:current_point, :delta_point, :current_gradient, :delta_gradient, :next_step_direction)) - 1
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:dzo_bfgs_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), getfield(o, :handle), w, p))
        return HipVector{T}(p[], getfield(o, :n))
    end
    return getfield(o, s)
end

################################################################################ AdGD

"""`AdGDOptimizer(constraint!, objective, gradient!, x0, initial_step_length)` (src/DZOptimization.jl:245-272) or the full
form with `f0, g0` (:203-243).  The struct of :179-200: the three callbacks are fields, the state fields are read
through `getproperty`.  `objective` may be a `BuiltinProblem` (then the step runs on the device's fused pass).  Aliases
`x0` as `current_point` and `g0` as `current_gradient` (:232, :235)."""
mutable struct AdGDOptimizer{T,A,C,F,G} <: AbstractOptimizer{T,A}
    handle::Ptr{Cvoid}
    constraint_function!::C
    objective_function::F
    gradient_function!::G
    current_point::A
    keep::Any
    AdGDOptimizer{T,A,C,F,G}(h, c, f, g, x, keep) where {T,A,C,F,G} =
        finalizer(o -> ccall((:dzo_adgd_destroy, libdzo), Cint, (Ptr{Cvoid},), getfield(o, :handle)), new{T,A,C,F,G}(h, c, f, g, x, keep))
end
# full form (:203-243)
function AdGDOptimizer(constraint!::C, objective::F, gradient!::G, x0::HipVector{T}, f0::Real, g0::HipVector{T},
                       initial_step_length::Real) where {T,C,F,G}
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_adgd_create, libdzo), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ref{Ptr{Cvoid}}),
                length(x0), dtype_code(T), x0.ptr, g0.ptr, f0, initial_step_length, h))
    cb = Ref(Callbacks{C,F,G,T}(constraint!, objective, gradient!, length(x0)))
    cf = constraint! === nothing ? C_NULL : @cfunction(_c_constraint, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
    check(ccall((:dzo_adgd_set_callbacks, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                h[], cf, @cfunction(_c_objective, Cdouble, (Ptr{Cvoid}, Ptr{Cvoid})),
                @cfunction(_c_gradient, Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), pointer_from_objref(cb)))
    return AdGDOptimizer{T,HipVector{T},C,F,G}(h[], constraint!, objective, gradient!, x0, (cb, g0))
end
# short form (:245-272)
function AdGDOptimizer(constraint!::C, objective::F, gradient!::G, x0::HipVector{T}, initial_step_length::Real) where {T,C,F,G}
    ensure_init()
    if objective isa BuiltinProblem && constraint! === nothing
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:dzo_adgd_create_problem, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}), objective.handle, x0.ptr, initial_step_length, h))
        return AdGDOptimizer{T,HipVector{T},C,F,G}(h[], constraint!, objective, gradient!, x0, objective)
    end
    if constraint! !== nothing
        @assert constraint!(x0)                                                    # :256-258
    end
    f0 = objective(x0)                                                             # :260
    g0 = similar(x0)                                                               # :262
    objective isa BuiltinProblem ? gradient!(objective, g0, x0) : gradient!(g0, x0)   # :265
    return AdGDOptimizer(constraint!, objective, objective isa BuiltinProblem ? ((g, x) -> gradient!(objective, g, x)) : gradient!,
                         x0, f0, g0, initial_step_length)
end
step!(opt::AdGDOptimizer) = (check(ccall((:dzo_adgd_step, libdzo), Cint, (Ptr{Cvoid},), getfield(opt, :handle))); opt)
_ad_i(o, w) = (v = Ref{Int64}(0); check(ccall((:dzo_adgd_get_i, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), getfield(o, :handle), w, v)); v[])
_ad_s(o, w) = (v = Ref{Cdouble}(0); check(ccall((:dzo_adgd_get_s, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), getfield(o, :handle), w, v)); v[])
# public fields of src/DZOptimization.jl:179-200
function Base.getproperty(o::AdGDOptimizer{T,A,C,F,G}, s::Symbol) where {T,A,C,F,G}
    s in (:is_stuck, :has_terminated, :has_converged) && return fill(_ad_i(o, 0) != 0)
    s === :iteration_count && return fill(Int(_ad_i(o, 1)))
    s === :current_objective_value && return fill(T(_ad_s(o, 0)))
    s === :delta_objective_value && return fill(T(_ad_s(o, 1)))
    s === :current_step_size && return fill(T(_ad_s(o, 2)))
    s === :previous_step_size && return fill(T(_ad_s(o, 3)))
    if s in (:delta_point, :current_gradient, :delta_gradient)
        # re-fetched on every access: delta_gradient moves between two buffers from step to step, and the
        # library re-reads what it cached about an array whose pointer was handed out (include/dzo.h)
        w = findfirst(==(s), (:current_point, :delta_point, :current_gradient, :delta_gradient)) - 1
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:dzo_adgd_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), getfield(o, :handle), w, p))
        return HipVector{T}(p[], length(getfield(o, :current_point)))
    end
    return getfield(o, s)
end

function read_field(o::AdGDOptimizer{T}, s::Symbol) where {T}       # (dzo_adgd_read: the same, for AdGD's four vector fields)
    w = findfirst(==(s), (:current_point, :delta_point, :current_gradient, :delta_gradient))
    w === nothing && throw(ArgumentError("read_field: unknown field $s"))
    out = Vector{T}(undef, length(getfield(o, :current_point)))
    check(ccall((:dzo_adgd_read, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), getfield(o, :handle), w - 1, out))
    return out
end

################################################################################ batched dense BFGS

"""`BatchedBFGSOptimizer(kind, x0, n, initial_step_length)`: `length(x0) / n` independent `BFGSOptimizer`s
(legacy/DZOptimization.jl:733-994 each) on one device, `x0` instance-major; `kind` = 1 for the chained
Rosenbrock objective.  `step!(b, k)` runs k synchronous steps of every live instance;
`count_active(b) == 0` is the shard's "everyone has_terminated".  One shard per process / GPU."""
mutable struct BatchedBFGSOptimizer{T}
    handle::Ptr{Cvoid}
    batch::Int
    n::Int
    function BatchedBFGSOptimizer(kind::Union{Integer,BuiltinProblem}, x0::HipVector{T}, n::Integer, step::Real; device::Union{Nothing,Integer}=nothing,
                                  matrices::Union{Nothing,HipVector{T}}=nothing) where {T}
        ensure_init()
        h = Ref{Ptr{Cvoid}}(C_NULL)
        batch = div(length(x0), n)
        if matrices !== nothing         # one symmetric n x n matrix per instance (instance-major); the caller keeps `matrices` alive
            check(ccall((:dzo_bfgs_batch_create_problem_matrices, libdzo), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                        kind.handle, batch, matrices.ptr, n * n, x0.ptr, step, device === nothing ? -1 : device, h))
        elseif kind isa BuiltinProblem      # objective, shared A of the quadratic and the decorators from the problem handle
            check(ccall((:dzo_bfgs_batch_create_problem, libdzo), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                        kind.handle, batch, x0.ptr, step, device === nothing ? -1 : device, h))
        elseif device === nothing
            check(ccall((:dzo_bfgs_batch_create, libdzo), Cint, (Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                        kind, batch, n, dtype_code(T), x0.ptr, step, h))
        else   # a shard on an explicit GPU (x0 must live there: `init(device); x0 = HipVector(...)`)
            check(ccall((:dzo_bfgs_batch_create_on, libdzo), Cint, (Cint, Cint, Int64, Int64, Cint, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                        device, kind, batch, n, dtype_code(T), x0.ptr, step, h))
        end
        return finalizer(o -> ccall((:dzo_bfgs_batch_destroy, libdzo), Cint, (Ptr{Cvoid},), getfield(o, :handle)),
                         new{T}(h[], batch, n))
    end
end

"""`ShardComm(devices)`: RCCL communicator over the GPUs of one node for ONE host process
(`ncclCommInitAll` behind `dzo_comm_init_all`); `ShardComm(id, nranks, rank)` joins a
process-per-GPU communicator whose 128-byte `id = ShardComm.unique_id()` rank 0 created.  The only
collective of the design is the convergence flag: `all_done(comm, shards)` is true when every instance of
every shard `has_terminated` (`dzo_bfgs_batch_all_done`: local counts + one 4-byte all-reduce(MIN) over
xGMI).  "run multiple optimizers in parallel" (README.md:12):

    comm   = ShardComm(0:7)
    shards = [ (init(d); BatchedBFGSOptimizer(1, HipVector(x0[d]), 256, 1.0; device=d)) for d in 0:7 ]
    while !all_done(comm, shards); foreach(s -> step!(s, 10), shards); end
"""
mutable struct ShardComm
    handle::Ptr{Cvoid}
    ShardComm(h::Ptr{Cvoid}) = finalizer(c -> ccall((:dzo_comm_destroy, libdzo), Cint, (Ptr{Cvoid},), c.handle), new(h))
end
function ShardComm(devices::AbstractVector{<:Integer})
    h = Ref{Ptr{Cvoid}}(C_NULL)
    devs = Cint.(collect(devices))
    check(ccall((:dzo_comm_init_all, libdzo), Cint, (Ptr{Cint}, Cint, Ref{Ptr{Cvoid}}), devs, length(devs), h))
    _initialised[] = true
    return ShardComm(h[])
end
function unique_id()
    ensure_init()
    id = Vector{UInt8}(undef, 128)
    check(ccall((:dzo_comm_unique_id, libdzo), Cint, (Ptr{UInt8},), id))
    return id
end
function ShardComm(id::Vector{UInt8}, nranks::Integer, rank::Integer)
    ensure_init()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_comm_init_rank, libdzo), Cint, (Ptr{UInt8}, Cint, Cint, Ref{Ptr{Cvoid}}), id, nranks, rank, h))
    return ShardComm(h[])
end
function all_done(comm::Union{ShardComm,Nothing}, shards::AbstractVector{<:BatchedBFGSOptimizer})
    hs = Ptr{Cvoid}[s.handle for s in shards]
    r = Ref{Cint}(0)
    check(ccall((:dzo_bfgs_batch_all_done, libdzo), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Ref{Cint}),
                comm === nothing ? C_NULL : comm.handle, hs, length(hs), r))
    return r[] != 0
end
"""`allreduce_min(comm, local_flags)`: the raw 4-byte collective (one flag per local rank)."""
function allreduce_min(comm::ShardComm, local_flags::AbstractVector{<:Integer})
    fl = Cint.(collect(local_flags)); r = Ref{Cint}(0)
    check(ccall((:dzo_flag_allreduce_min_n, libdzo), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Ref{Cint}), comm.handle, fl, length(fl), r))
    return Int(r[])
end
step!(b::BatchedBFGSOptimizer, steps::Integer=1) =
    (check(ccall((:dzo_bfgs_batch_step, libdzo), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), b.handle, steps, C_NULL)); b)
"""`set_max_increases!(b, k)`: `QuadraticLineSearch.max_increases` (legacy/DZOptimization.jl:181-188) of every instance."""
set_max_increases!(b::BatchedBFGSOptimizer, k::Integer) =
    (check(ccall((:dzo_bfgs_batch_set_max_increases, libdzo), Cint, (Ptr{Cvoid}, Cint), b.handle, k)); b)
function count_active(b::BatchedBFGSOptimizer)
    v = Ref{Int64}(0)
    check(ccall((:dzo_bfgs_batch_count_active, libdzo), Cint, (Ptr{Cvoid}, Ref{Int64}), b.handle, v))
    return Int(v[])
end
"""`current_point(b)`: the batch x n points (instance-major) as one device vector."""
function current_point(b::BatchedBFGSOptimizer{T}) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dzo_bfgs_batch_get_ptr, libdzo), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), b.handle, 0, p))
    return HipVector{T}(p[], b.batch * b.n)
end

################################################################################ LineSearchEvaluator

"""`LineSearchEvaluator(constraint!, objective, gradient!, x, f, d, overlap)` and its call
`ev(t, compute_gradient)` -> `(trial_objective_value, improvement_ratio, slope_ratio)`
(src/DZOptimization.jl:12-62, :65-92).  `trial_point` / `trial_gradient` are the evaluator's own."""
struct LineSearchEvaluator{T,CB}
    callbacks::CB
    current_point::HipVector{T}
    current_objective_value::T
    step_direction::HipVector{T}
    overlap::T
    trial_point::HipVector{T}
    trial_gradient::HipVector{T}
end
function LineSearchEvaluator(constraint!::C, objective::F, gradient!::G, x::HipVector{T}, f::Real, d::HipVector{T},
                             overlap::Real) where {T,C,F,G}
    cb = Ref(Callbacks{C,F,G,T}(constraint!, objective, gradient!, length(x)))
    return LineSearchEvaluator{T,typeof(cb)}(cb, x, T(f), d, T(overlap), similar(x), similar(x))
end
function (ev::LineSearchEvaluator{T})(step_size::Real, compute_gradient::Bool) where {T}
    cb = ev.callbacks
    cf = cb[].constraint! === nothing ? C_NULL : @cfunction(_c_constraint, Cint, (Ptr{Cvoid}, Ptr{Cvoid}))
    f, imp, slope = Ref{Cdouble}(0), Ref{Cdouble}(0), Ref{Cdouble}(0)
    GC.@preserve cb check(ccall((:dzo_line_search_eval, libdzo), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Cdouble, Ptr{Cvoid}, Cdouble, Cdouble,
                 Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cdouble}),
                cf, @cfunction(_c_objective, Cdouble, (Ptr{Cvoid}, Ptr{Cvoid})),
                @cfunction(_c_gradient, Cvoid, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), pointer_from_objref(cb),
                length(ev.current_point), dtype_code(T), ev.current_point.ptr, ev.current_objective_value,
                ev.step_direction.ptr, ev.overlap, step_size, compute_gradient, ev.trial_point.ptr,
                ev.trial_gradient.ptr, f, imp, slope))
    return T(f[]), T(imp[]), T(slope[])
end

end # module
