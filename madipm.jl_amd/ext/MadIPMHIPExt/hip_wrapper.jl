# ROCArray methods of MadIPM / MadNLP / NLPModels over libmadipm_hip.so (include/madipm_hip.h).
#
# Counterpart of the reference's ext/MadIPMCUDAExt/cuda_wrapper.jl: every kernel of that file is
# replaced by a C-ABI entry point of csrc/kkt.hip (hand-written gfx950 HIP, fixed summation orders).
# The C-ABI is 0-based; Julia's sparse device matrices are 1-based, so index arrays are shifted once
# (structure arrays never change after construction: `zero_based` caches the shifted copy per array)
# while value arrays are passed through untouched and read live.
#
# Not executed in this repository (no Julia toolchain in the image); the Python mirror
# madipm_amd/rocm_wrapper.py binds the same symbols and is what tests/test_kkt_ops_gpu.py runs.

const libmadipm = get(ENV, "MADIPM_HIP_LIB", joinpath(@__DIR__, "..", "..", "madipm_amd", "lib", "libmadipm_hip.so"))

function check(rc::Integer, what::AbstractString="libmadipm_hip")
    rc < 0 && error(what, ": ", unsafe_string(ccall((:madipm_last_error, libmadipm), Cstring, ())))
    return Int(rc)
end

hipstream() = AMDGPU.stream().stream                 # hipStream_t of the task-local stream

# Per-array caches keyed by object IDENTITY (objectid), never by content: hashing a device array would
# read it element by element from the host.  The entry is dropped by a finalizer on the key array.
function cached!(f, cache::Dict{UInt,Any}, x)
    id = objectid(x)
    v = get(cache, id, nothing)
    v === nothing || return v
    v = f()
    cache[id] = v
    finalizer(_ -> delete!(cache, id), x)
    return v
end

# 0-based copies of 1-based index arrays (structure arrays: never change after construction)
const ZB = Dict{UInt,Any}()
zero_based(x::ROCVector{Ti}) where {Ti<:Integer} = cached!(() -> x .- one(Ti), ZB, x)

# ------------------------------------------------------------ transfer!  (cuda_wrapper.jl:4-24)
mutable struct TransferPlan
    handle::Ptr{Cvoid}
    nsrc::Int
    ndest::Int
end
const PLANS = Dict{UInt,Any}()

function transfer_plan(map::ROCVector{Int}, ndest::Int)
    p = get(PLANS, objectid(map), nothing)
    (p !== nothing && p.ndest == ndest) && return p
    hmap = Int64.(Array(map)) .- 1                    # 0-based, host; counting-sorted by the library
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:madipm_transfer_create, libmadipm), Cint, (Int64, Ptr{Int64}, Int32, Int64, Ref{Ptr{Cvoid}}),
                length(hmap), hmap, Int32(0), ndest, h), "madipm_transfer_create")
    p = TransferPlan(h[], length(hmap), ndest)
    finalizer(q -> ccall((:madipm_transfer_destroy, libmadipm), Cvoid, (Ptr{Cvoid},), q.handle), p)
    p0 = get(PLANS, objectid(map), nothing)
    PLANS[objectid(map)] = p
    p0 === nothing && finalizer(_ -> delete!(PLANS, objectid(map)), map)
    return p
end

function MadNLP.transfer!(dest::ROCSparseMatrixCSC{Tv}, src::MadNLP.SparseMatrixCOO{Tv},
                          map::ROCVector{Int}) where {Tv<:Float64}
    # dest .= 0; dest[map[k]] += src[k], each entry summed in ascending k (deterministic)
    p = transfer_plan(map, length(nonzeros(dest)))
    GC.@preserve dest src check(ccall((:madipm_transfer, libmadipm), Cint,
                                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                                      p.handle, pointer(nonzeros(dest)), pointer(src.V), hipstream()), "madipm_transfer")
    return
end

function MadNLP.compress_hessian!(kkt::MadNLP.SparseKKTSystem{T,VT,MT}) where {T,VT,MT<:ROCSparseMatrixCSC{T,Int32}}
    MadNLP.transfer!(kkt.hess_com, kkt.hess_raw, kkt.hess_csc_map)
end

# ------------------------------------------------------------ compress_jacobian!  (cuda_wrapper.jl:32-41)
function MadNLP.compress_jacobian!(kkt::MadIPM.NormalKKTSystem{T,VT,MT}) where {T,VT,MT<:ROCSparseMatrixCSC{T,Int32}}
    n_slack = length(kkt.ind_ineq)
    map0 = zero_based(kkt.A_csr_map)
    GC.@preserve kkt map0 check(ccall((:madipm_compress_jacobian, libmadipm), Cint,
                                      (Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}),
                                      pointer(kkt.A.V), length(kkt.A.V), Int32(n_slack), pointer(map0),
                                      pointer(kkt.AT.nzVal), hipstream()), "madipm_compress_jacobian")
    return
end

# ------------------------------------------------------------ SpMV operator  (cuda_wrapper.jl:43-94)
mutable struct MadIPMOperator{T,M} <: AbstractMatrix{T}
    type::Type{T}
    m::Int
    n::Int
    A::M
    transa::Char
    handle::Ptr{Cvoid}
    rp0::ROCVector{Int32}                            # 0-based structure (values of A read live)
    ci0::ROCVector{Int32}
end

Base.eltype(A::MadIPMOperator{T}) where T = T
Base.size(A::MadIPMOperator) = (A.m, A.n)
SparseArrays.nnz(A::MadIPMOperator) = nnz(A.A)

function MadIPMOperator(A::ROCSparseMatrixCSR{T,Int32}; transa::Char='N', symmetric::Bool=false) where T<:Float64
    m, n = size(A)
    rp0, ci0 = A.rowPtr .- Int32(1), A.colVal .- Int32(1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A rp0 ci0 check(ccall((:madipm_spmv_create, libmadipm), Cint,
                                       (Int32, Int32, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, UInt8, Int32,
                                        Ref{Ptr{Cvoid}}),
                                       m, n, nnz(A), pointer(rp0), pointer(ci0), pointer(A.nzVal), UInt8(transa),
                                       Int32(symmetric), h), "madipm_spmv_create")
    op = MadIPMOperator{T,typeof(A)}(T, m, n, A, transa, h[], rp0, ci0)
    finalizer(o -> ccall((:madipm_spmv_destroy, libmadipm), Cvoid, (Ptr{Cvoid},), o.handle), op)
    return op
end
MadIPMOperator(A::ROCSparseMatrixCSC; kw...) = MadIPMOperator(ROCSparseMatrixCSR(A); kw...)
MadIPMOperator(A::ROCSparseMatrixCOO; kw...) = MadIPMOperator(ROCSparseMatrixCSR(A); kw...)

function LinearAlgebra.mul!(y::ROCVector{T}, A::MadIPMOperator{T}, x::ROCVector{T}, alpha::Number=one(T),
                            beta::Number=zero(T)) where T<:Float64
    GC.@preserve A x y check(ccall((:madipm_spmv_apply, libmadipm), Cint,
                                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Cvoid}),
                                   A.handle, pointer(x), pointer(y), Float64(alpha), Float64(beta), hipstream()),
                             "madipm_spmv_apply")
    return y
end

# ------------------------------------------------------------ coo_to_csr  (cuda_wrapper.jl:96-106)
function MadIPM.coo_to_csr(n_rows, n_cols, Ai::ROCVector{Ti}, Aj::ROCVector{Ti}, Ax::ROCVector{Tv}) where {Tv,Ti}
    @assert length(Ai) == length(Aj) == length(Ax)
    nz = length(Ai)
    Ai0, Aj0 = Int32.(Ai) .- Int32(1), Int32.(Aj) .- Int32(1)
    Bp, Bj, Bx = ROCVector{Int32}(undef, n_rows + 1), ROCVector{Int32}(undef, nz), ROCVector{Float64}(undef, nz)
    # columns sorted within a row: the layout the reference's sparse(...; fmt=:csr) produces
    Axf = Float64.(Ax)
    GC.@preserve Ai0 Aj0 Axf Bp Bj Bx check(ccall((:madipm_coo_to_csr, libmadipm), Cint,
        (Int32, Int32, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{Cvoid}),
        n_rows, n_cols, nz, pointer(Ai0), pointer(Aj0), pointer(Axf), pointer(Bp), pointer(Bj), pointer(Bx),
        Int32(1), hipstream()), "madipm_coo_to_csr")
    return (Ti.(Bp .+ Int32(1)), Ti.(Bj .+ Int32(1)), Tv.(Bx))
end

# ------------------------------------------------------------ normal equations  (cuda_wrapper.jl:108-234)
function MadIPM.assemble_normal_system!(n_rows, n_cols, Jtp::ROCArray{Ti}, Jtj::ROCArray{Ti}, Jtx::ROCArray{Tv},
                                        Cp::ROCArray{Ti}, Cj::ROCArray{Ti}, Cx::ROCArray{Tv},
                                        Dx::ROCArray{Tv}) where {Ti<:Int32,Tv<:Float64}
    Jtp0, Jtj0, Cp0, Cj0 = zero_based(Jtp), zero_based(Jtj), zero_based(Cp), zero_based(Cj)
    GC.@preserve Jtp0 Jtj0 Cp0 Cj0 Jtx Cx Dx check(ccall((:madipm_assemble_normal_system, libmadipm), Cint,
        (Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        n_rows, n_cols, pointer(Jtp0), pointer(Jtj0), pointer(Jtx), pointer(Cp0), pointer(Cj0), pointer(Cx),
        pointer(Dx), hipstream()), "madipm_assemble_normal_system")
    return
end

function MadIPM.build_normal_system(n_rows, n_cols, Jtp::ROCVector{Ti}, Jtj::ROCVector{Ti}) where {Ti}
    Jp, Jj = Int32.(Array(Jtp)) .- Int32(1), Int32.(Array(Jtj)) .- Int32(1)
    Cp = zeros(Int32, n_rows + 1)
    nz = Ref{Int64}(0)
    check(ccall((:madipm_build_normal_system, libmadipm), Cint,
                (Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}),
                n_rows, n_cols, Jp, Jj, Cp, C_NULL, 0, nz), "madipm_build_normal_system")
    Cj = zeros(Int32, nz[])
    check(ccall((:madipm_build_normal_system, libmadipm), Cint,
                (Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}),
                n_rows, n_cols, Jp, Jj, Cp, Cj, nz[], nz), "madipm_build_normal_system")
    return (ROCVector{Ti}(Cp .+ Int32(1)), ROCVector{Ti}(Cj .+ Int32(1)))
end

MadIPM.sparse_csc_format(::Type{<:ROCArray}) = ROCSparseMatrixCSC
MadIPM._colptr(A::ROCSparseMatrixCSC) = A.colPtr
MadIPM._rowval(A::ROCSparseMatrixCSC) = A.rowVal
MadIPM._nzval(A::ROCSparseMatrixCSC) = A.nzVal

# ------------------------------------------------------------ re-solve with new numbers  (madipm_hip.h, ABI 0.2.4)
# madipm_qp_update: host pointers read during the call only; C_NULL keeps the solver's current data.
# Lengths are the creation-time nvar / ncon / nnzj / nnzh, Hvals / Avals in the creation-time COO order.
struct MadipmQPUpdate
    c::Ptr{Float64}
    c0::Ptr{Float64}          # a pointer, so that C_NULL means "keep"
    Hvals::Ptr{Float64}
    Avals::Ptr{Float64}
    lcon::Ptr{Float64}
    ucon::Ptr{Float64}
    lvar::Ptr{Float64}
    uvar::Ptr{Float64}
    x0::Ptr{Float64}
    y0::Ptr{Float64}
end

_ptr_or_null(a::Nothing) = Ptr{Float64}(C_NULL)
_ptr_or_null(a::Vector{Float64}) = pointer(a)

# Builds the refresh plan once, from the Ref{MadipmQP} the solver was created with (a second call is a no-op).
function solver_prepare_update(h::Ptr{Cvoid}, q::Base.RefValue)
    GC.@preserve q check(ccall((:madipm_solver_prepare_update, libmadipm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}),
                               h, Base.unsafe_convert(Ptr{Cvoid}, q)), "madipm_solver_prepare_update")
    return
end

# Installs new numbers; the next madipm_solver_solve runs on the updated problem from its x0 / y0.  An error
# (a change of the classification of a bound; no prepare_update) leaves the solver as it was.
function solver_update(h::Ptr{Cvoid}; c=nothing, c0=nothing, Hvals=nothing, Avals=nothing, lcon=nothing,
                       ucon=nothing, lvar=nothing, uvar=nothing, x0=nothing, y0=nothing)
    c0v = c0 === nothing ? nothing : Float64[c0]
    GC.@preserve c c0v Hvals Avals lcon ucon lvar uvar x0 y0 begin
        u = Ref(MadipmQPUpdate(_ptr_or_null(c), _ptr_or_null(c0v), _ptr_or_null(Hvals), _ptr_or_null(Avals),
                               _ptr_or_null(lcon), _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar),
                               _ptr_or_null(x0), _ptr_or_null(y0)))
        check(ccall((:madipm_solver_update, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmQPUpdate}), h, u),
              "madipm_solver_update")
    end
    return
end

# (n_analyses, n_updates, last_update_s): analyses run for this solver (stays 1), successful updates, host
# wall time of the last one
function solver_counters(h::Ptr{Cvoid})
    na, nu, t = Ref{Int64}(0), Ref{Int64}(0), Ref{Float64}(0.0)
    check(ccall((:madipm_solver_counters, libmadipm), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Float64}),
                h, na, nu, t), "madipm_solver_counters")
    return (n_analyses = na[], n_updates = nu[], last_update_s = t[])
end

# ---- the device route (ABI 0.2.5): the update reads DEVICE arrays, the solution is written to DEVICE arrays.
# The arrays are Ptr{Float64} into device memory (e.g. pointer(::ROCArray{Float64})), or nothing = keep;
# c0 stays a host number.  `stream` is the HIP stream the arrays were produced on (C_NULL: the default
# stream): the reads are ordered after the work enqueued on it, and the call returns with its reads done.
_dptr_or_null(a::Nothing) = Ptr{Float64}(C_NULL)
_dptr_or_null(a::Ptr{Float64}) = a

function solver_update_device(h::Ptr{Cvoid}; c=nothing, c0=nothing, Hvals=nothing, Avals=nothing, lcon=nothing,
                              ucon=nothing, lvar=nothing, uvar=nothing, x0=nothing, y0=nothing,
                              stream::Ptr{Cvoid}=C_NULL)
    c0v = c0 === nothing ? nothing : Float64[c0]
    GC.@preserve c0v begin
        u = Ref(MadipmQPUpdate(_dptr_or_null(c), _ptr_or_null(c0v), _dptr_or_null(Hvals), _dptr_or_null(Avals),
                               _dptr_or_null(lcon), _dptr_or_null(ucon), _dptr_or_null(lvar), _dptr_or_null(uvar),
                               _dptr_or_null(x0), _dptr_or_null(y0)))
        check(ccall((:madipm_solver_update_device, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmQPUpdate}, Ptr{Cvoid}),
                    h, u, stream), "madipm_solver_update_device")
    end
    return
end

# update_solution! into device arrays (any may be C_NULL); does not block the host, work enqueued on `stream`
# afterwards sees the values
function solver_get_solution_device(h::Ptr{Cvoid}, d_x::Ptr{Float64}, d_y::Ptr{Float64}, d_zl::Ptr{Float64},
                                    d_zu::Ptr{Float64}, d_cons::Ptr{Float64}; stream::Ptr{Cvoid}=C_NULL)
    check(ccall((:madipm_solver_get_solution_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h, d_x, d_y, d_zl, d_zu, d_cons, stream), "madipm_solver_get_solution_device")
    return
end

# the raw problem numbers the solver holds, into host vectors of the creation-time lengths (nothing = skip);
# returns c0
function solver_get_data(h::Ptr{Cvoid}; c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing, ucon=nothing,
                         lvar=nothing, uvar=nothing, x0=nothing, y0=nothing)
    c0 = Ref{Float64}(0.0)
    GC.@preserve c Hvals Avals lcon ucon lvar uvar x0 y0 begin
        check(ccall((:madipm_solver_get_data, libmadipm), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    h, _ptr_or_null(c), c0, _ptr_or_null(Hvals), _ptr_or_null(Avals), _ptr_or_null(lcon),
                    _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar), _ptr_or_null(x0), _ptr_or_null(y0)),
              "madipm_solver_get_data")
    end
    return c0[]
end

# ---- warm start (ABI 0.2.6): the following solves start from a point (x, y, zl, zu) of the public, un-scaled
# space (what solver_get_solution returns; lengths nvar, ncon, nvar, nvar; nothing = the block keeps its
# cold values, not all four) blended into the cold start with `weight` in (0, 1).  The point persists across
# solves and updates until it is replaced or cleared.  Non-finite entries are not checked.
function solver_set_warm_start(h::Ptr{Cvoid}; x=nothing, y=nothing, zl=nothing, zu=nothing, weight::Real=0.99)
    GC.@preserve x y zl zu begin
        check(ccall((:madipm_solver_set_warm_start, libmadipm), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble),
                    h, _ptr_or_null(x), _ptr_or_null(y), _ptr_or_null(zl), _ptr_or_null(zu), Float64(weight)),
              "madipm_solver_set_warm_start")
    end
    return
end

# the same from DEVICE arrays (Ptr{Float64} into device memory, or nothing) produced on `stream`: the reads
# are ordered after the work enqueued on it, the host is not synchronised, and work enqueued on `stream`
# afterwards (overwriting the arrays) is ordered after the copies
function solver_set_warm_start_device(h::Ptr{Cvoid}; x=nothing, y=nothing, zl=nothing, zu=nothing,
                                      weight::Real=0.99, stream::Ptr{Cvoid}=C_NULL)
    check(ccall((:madipm_solver_set_warm_start_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Cvoid}),
                h, _dptr_or_null(x), _dptr_or_null(y), _dptr_or_null(zl), _dptr_or_null(zu), Float64(weight), stream),
          "madipm_solver_set_warm_start_device")
    return
end

# the solver's own current iterate as the warm point, without leaving the device (an error before the first
# solve); in a re-solve loop: solve, solver_warm_start_last, update, solve
function solver_warm_start_last(h::Ptr{Cvoid}; weight::Real=0.99)
    check(ccall((:madipm_solver_warm_start_last, libmadipm), Cint, (Ptr{Cvoid}, Cdouble), h, Float64(weight)),
          "madipm_solver_warm_start_last")
    return
end

function solver_clear_warm_start(h::Ptr{Cvoid})
    check(ccall((:madipm_solver_clear_warm_start, libmadipm), Cint, (Ptr{Cvoid},), h),
          "madipm_solver_clear_warm_start")
    return
end

# (active, weight, n_warm_inits): a point is set, its weight, initialisations that blended
function solver_warm_info(h::Ptr{Cvoid})
    a, w, k = Ref{Int32}(0), Ref{Float64}(0.0), Ref{Int64}(0)
    check(ccall((:madipm_solver_warm_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Float64}, Ref{Int64}),
                h, a, w, k), "madipm_solver_warm_info")
    return (active = a[] != 0, weight = w[], n_warm_inits = k[])
end

# ---- adjoint gradients (ABI 0.2.7): for a loss l(x*) of the last successful solve's x* alone, given
# gx = dl/dx* (length nvar), the gradients of l with respect to the data.  madipm_qp_gradients: seven
# pointers (c, Hvals, Avals, lcon, ucon, lvar, uvar; lengths nvar, nnzh, nnzj, ncon, ncon, nvar, nvar), a null
# one = not wanted.  K2 only; refused before a solve, after an update no solve followed, on a failed solve.
struct MadipmQPGradients
    c::Ptr{Float64}
    Hvals::Ptr{Float64}
    Avals::Ptr{Float64}
    lcon::Ptr{Float64}
    ucon::Ptr{Float64}
    lvar::Ptr{Float64}
    uvar::Ptr{Float64}
end

# HOST vectors (or nothing); the outputs are written during the call
function solver_adjoint(h::Ptr{Cvoid}, gx::Vector{Float64}; c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing,
                        ucon=nothing, lvar=nothing, uvar=nothing)
    GC.@preserve gx c Hvals Avals lcon ucon lvar uvar begin
        g = Ref(MadipmQPGradients(_ptr_or_null(c), _ptr_or_null(Hvals), _ptr_or_null(Avals), _ptr_or_null(lcon),
                                  _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar)))
        check(ccall((:madipm_solver_adjoint, libmadipm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{MadipmQPGradients}),
                    h, pointer(gx), g), "madipm_solver_adjoint")
    end
    return
end

# DEVICE arrays (Ptr{Float64} into device memory, or nothing): gx is read after the work enqueued on `stream`,
# and work enqueued on `stream` after the call sees the outputs
function solver_adjoint_device(h::Ptr{Cvoid}, gx::Ptr{Float64}; c=nothing, Hvals=nothing, Avals=nothing,
                               lcon=nothing, ucon=nothing, lvar=nothing, uvar=nothing, stream::Ptr{Cvoid}=C_NULL)
    g = Ref(MadipmQPGradients(_dptr_or_null(c), _dptr_or_null(Hvals), _dptr_or_null(Avals), _dptr_or_null(lcon),
                              _dptr_or_null(ucon), _dptr_or_null(lvar), _dptr_or_null(uvar)))
    check(ccall((:madipm_solver_adjoint_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ref{MadipmQPGradients}, Ptr{Cvoid}), h, gx, g, stream),
          "madipm_solver_adjoint_device")
    return
end

# (n_adjoints, n_adjoint_factorizations, last_residual): successful calls, those that factorised (one per
# solved point), and the last call's ||g - K a||_inf / max(1, ||g||_inf)
function solver_adjoint_info(h::Ptr{Cvoid})
    na, nf, r = Ref{Int64}(0), Ref{Int64}(0), Ref{Float64}(0.0)
    check(ccall((:madipm_solver_adjoint_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Float64}),
                h, na, nf, r), "madipm_solver_adjoint_info")
    return (n_adjoints = na[], n_adjoint_factorizations = nf[], last_residual = r[])
end

# ---- adjoint of all five solution blocks (ABI 0.2.8): the loss is l(x, y, zl, zu, A x).  madipm_qp_cotangents:
# five pointers (x, y, zl, zu, cons; lengths nvar, ncon, nvar, nvar, ncon), a null one = absent (0), not all
# five.  zl / zu of a variable without that bound and of a fixed variable are constants: their cotangents are
# not read.  Outputs, conventions and refusals are solver_adjoint's; with gx alone the bits are its bits.
struct MadipmQPCotangents
    x::Ptr{Float64}
    y::Ptr{Float64}
    zl::Ptr{Float64}
    zu::Ptr{Float64}
    cons::Ptr{Float64}
end

# HOST vectors (or nothing)
function solver_adjoint_full(h::Ptr{Cvoid}; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing, gcons=nothing,
                             c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing, ucon=nothing, lvar=nothing,
                             uvar=nothing)
    GC.@preserve gx gy gzl gzu gcons c Hvals Avals lcon ucon lvar uvar begin
        ct = Ref(MadipmQPCotangents(_ptr_or_null(gx), _ptr_or_null(gy), _ptr_or_null(gzl), _ptr_or_null(gzu),
                                    _ptr_or_null(gcons)))
        g = Ref(MadipmQPGradients(_ptr_or_null(c), _ptr_or_null(Hvals), _ptr_or_null(Avals), _ptr_or_null(lcon),
                                  _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar)))
        check(ccall((:madipm_solver_adjoint_full, libmadipm), Cint,
                    (Ptr{Cvoid}, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}), h, ct, g),
              "madipm_solver_adjoint_full")
    end
    return
end

# DEVICE arrays (Ptr{Float64} into device memory, or nothing), with solver_adjoint_device's stream contract
function solver_adjoint_full_device(h::Ptr{Cvoid}; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing, gcons=nothing,
                                    c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing, ucon=nothing,
                                    lvar=nothing, uvar=nothing, stream::Ptr{Cvoid}=C_NULL)
    ct = Ref(MadipmQPCotangents(_dptr_or_null(gx), _dptr_or_null(gy), _dptr_or_null(gzl), _dptr_or_null(gzu),
                                _dptr_or_null(gcons)))
    g = Ref(MadipmQPGradients(_dptr_or_null(c), _dptr_or_null(Hvals), _dptr_or_null(Avals), _dptr_or_null(lcon),
                              _dptr_or_null(ucon), _dptr_or_null(lvar), _dptr_or_null(uvar)))
    check(ccall((:madipm_solver_adjoint_full_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}, Ptr{Cvoid}), h, ct, g, stream),
          "madipm_solver_adjoint_full_device")
    return
end

# ---- polish: the exact active-set solve after the interior-point method (ABI 0.2.10).  The active set the end
# point identifies (or the caller's: one Int8 per variable and one per row, -1 lower, +1 upper, 0 inactive), the
# active coordinates at their bounds, the equality-constrained QP of that face solved to rounding level.
# madipm_polish_out: seven pointers (x, y, zl, zu, cons: Float64; active_var, active_row: Int8), a null one = not
# wanted, not all seven.  The verdict (0 polished, 1 wrong set, 2 no convergence, 3 factorisation failed) comes
# back in the info; with a verdict other than 0 the blocks are solver_get_solution's.
struct MadipmPolishOpts
    sigma::Float64
    tol_resid::Float64
    tol_sign::Float64
    tol_feas::Float64
    refine_steps::Int32
end
struct MadipmPolishOut
    x::Ptr{Float64}
    y::Ptr{Float64}
    zl::Ptr{Float64}
    zu::Ptr{Float64}
    cons::Ptr{Float64}
    active_var::Ptr{Int8}
    active_row::Ptr{Int8}
end
struct MadipmPolishInfo
    verdict::Int32
    n_active::Int32
    residual::Float64
    min_multiplier::Float64
    min_gap::Float64
    n_polishes::Int64
    n_polish_factorizations::Int64
end
MadipmPolishInfo() = MadipmPolishInfo(-1, 0, 0.0, 0.0, 0.0, 0, 0)

function polish_default_opts()
    o = Ref(MadipmPolishOpts(0.0, 0.0, 0.0, 0.0, 0))
    ccall((:madipm_polish_default_opts, libmadipm), Cvoid, (Ref{MadipmPolishOpts},), o)
    return o[]
end

_i8ptr_or_null(a::Nothing) = Ptr{Int8}(C_NULL)
_i8ptr_or_null(a::Vector{Int8}) = pointer(a)
_i8ptr_or_null(a::Ptr{Int8}) = a

# host arrays: Vector{Float64} / Vector{Int8} of the right lengths, or nothing
function solver_polish(h::Ptr{Cvoid}; opts::MadipmPolishOpts=polish_default_opts(), active_var=nothing,
                       active_row=nothing, x=nothing, y=nothing, zl=nothing, zu=nothing, cons=nothing,
                       out_active_var=nothing, out_active_row=nothing)
    info = Ref(MadipmPolishInfo())
    GC.@preserve active_var active_row x y zl zu cons out_active_var out_active_row begin
        o = Ref(MadipmPolishOut(_ptr_or_null(x), _ptr_or_null(y), _ptr_or_null(zl), _ptr_or_null(zu),
                                _ptr_or_null(cons), _i8ptr_or_null(out_active_var), _i8ptr_or_null(out_active_row)))
        check(ccall((:madipm_solver_polish, libmadipm), Cint,
                    (Ptr{Cvoid}, Ref{MadipmPolishOpts}, Ptr{Int8}, Ptr{Int8}, Ref{MadipmPolishOut},
                     Ref{MadipmPolishInfo}),
                    h, Ref(opts), _i8ptr_or_null(active_var), _i8ptr_or_null(active_row), o, info),
              "madipm_solver_polish")
    end
    return info[]
end

# device arrays: Ptr{Float64} / Ptr{Int8} into device memory, or nothing; the stream contract of
# solver_adjoint_device.  The info comes back on the host.
function solver_polish_device(h::Ptr{Cvoid}; opts::MadipmPolishOpts=polish_default_opts(), active_var=nothing,
                              active_row=nothing, x=nothing, y=nothing, zl=nothing, zu=nothing, cons=nothing,
                              out_active_var=nothing, out_active_row=nothing, stream::Ptr{Cvoid}=C_NULL)
    info = Ref(MadipmPolishInfo())
    o = Ref(MadipmPolishOut(_dptr_or_null(x), _dptr_or_null(y), _dptr_or_null(zl), _dptr_or_null(zu),
                            _dptr_or_null(cons), _i8ptr_or_null(out_active_var), _i8ptr_or_null(out_active_row)))
    check(ccall((:madipm_solver_polish_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{MadipmPolishOpts}, Ptr{Int8}, Ptr{Int8}, Ref{MadipmPolishOut}, Ref{MadipmPolishInfo},
                 Ptr{Cvoid}),
                h, Ref(opts), _i8ptr_or_null(active_var), _i8ptr_or_null(active_row), o, info, stream),
          "madipm_solver_polish_device")
    return info[]
end

function solver_polish_info(h::Ptr{Cvoid})
    info = Ref(MadipmPolishInfo())
    check(ccall((:madipm_solver_polish_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmPolishInfo}), h, info),
          "madipm_solver_polish_info")
    return info[]
end

# ---- sensitivities at the polished point (ABI 0.2.11): the exact derivatives of the face the last solver_polish
# of this solved point ended polished on (verdict 0; refused otherwise, and before any polish).  The tangent's
# structs have the layouts of the adjoint's: madipm_qp_directions is seven pointers (c, Hvals, Avals, lcon, ucon,
# lvar, uvar), madipm_qp_point_tangents five (x, y, zl, zu, cons); a null one = 0 / not wanted.  The tangent of
# an active variable is its bound's direction, zl / zu of an inactive bound move by exactly 0, the gradient of
# an inactive bound is exactly 0.
const MadipmQPDirections = MadipmQPGradients
const MadipmQPPointTangents = MadipmQPCotangents

# HOST vectors (or nothing): directions dc ... duvar in, dx ... dcons out
function solver_tangent_polished(h::Ptr{Cvoid}; dc=nothing, dHvals=nothing, dAvals=nothing, dlcon=nothing,
                                 ducon=nothing, dlvar=nothing, duvar=nothing, x=nothing, y=nothing, zl=nothing,
                                 zu=nothing, cons=nothing)
    GC.@preserve dc dHvals dAvals dlcon ducon dlvar duvar x y zl zu cons begin
        d = Ref(MadipmQPDirections(_ptr_or_null(dc), _ptr_or_null(dHvals), _ptr_or_null(dAvals), _ptr_or_null(dlcon),
                                   _ptr_or_null(ducon), _ptr_or_null(dlvar), _ptr_or_null(duvar)))
        o = Ref(MadipmQPPointTangents(_ptr_or_null(x), _ptr_or_null(y), _ptr_or_null(zl), _ptr_or_null(zu),
                                      _ptr_or_null(cons)))
        check(ccall((:madipm_solver_tangent_polished, libmadipm), Cint,
                    (Ptr{Cvoid}, Ref{MadipmQPDirections}, Ref{MadipmQPPointTangents}), h, d, o),
              "madipm_solver_tangent_polished")
    end
    return
end

# DEVICE arrays (Ptr{Float64} into device memory, or nothing), with solver_adjoint_device's stream contract
function solver_tangent_polished_device(h::Ptr{Cvoid}; dc=nothing, dHvals=nothing, dAvals=nothing, dlcon=nothing,
                                        ducon=nothing, dlvar=nothing, duvar=nothing, x=nothing, y=nothing,
                                        zl=nothing, zu=nothing, cons=nothing, stream::Ptr{Cvoid}=C_NULL)
    d = Ref(MadipmQPDirections(_dptr_or_null(dc), _dptr_or_null(dHvals), _dptr_or_null(dAvals), _dptr_or_null(dlcon),
                               _dptr_or_null(ducon), _dptr_or_null(dlvar), _dptr_or_null(duvar)))
    o = Ref(MadipmQPPointTangents(_dptr_or_null(x), _dptr_or_null(y), _dptr_or_null(zl), _dptr_or_null(zu),
                                  _dptr_or_null(cons)))
    check(ccall((:madipm_solver_tangent_polished_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{MadipmQPDirections}, Ref{MadipmQPPointTangents}, Ptr{Cvoid}), h, d, o, stream),
          "madipm_solver_tangent_polished_device")
    return
end

# HOST vectors (or nothing): the arguments of solver_adjoint_full
function solver_adjoint_polished(h::Ptr{Cvoid}; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing, gcons=nothing,
                                 c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing, ucon=nothing, lvar=nothing,
                                 uvar=nothing)
    GC.@preserve gx gy gzl gzu gcons c Hvals Avals lcon ucon lvar uvar begin
        ct = Ref(MadipmQPCotangents(_ptr_or_null(gx), _ptr_or_null(gy), _ptr_or_null(gzl), _ptr_or_null(gzu),
                                    _ptr_or_null(gcons)))
        g = Ref(MadipmQPGradients(_ptr_or_null(c), _ptr_or_null(Hvals), _ptr_or_null(Avals), _ptr_or_null(lcon),
                                  _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar)))
        check(ccall((:madipm_solver_adjoint_polished, libmadipm), Cint,
                    (Ptr{Cvoid}, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}), h, ct, g),
              "madipm_solver_adjoint_polished")
    end
    return
end

# DEVICE arrays (Ptr{Float64} into device memory, or nothing), with solver_adjoint_device's stream contract
function solver_adjoint_polished_device(h::Ptr{Cvoid}; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing,
                                        gcons=nothing, c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing,
                                        ucon=nothing, lvar=nothing, uvar=nothing, stream::Ptr{Cvoid}=C_NULL)
    ct = Ref(MadipmQPCotangents(_dptr_or_null(gx), _dptr_or_null(gy), _dptr_or_null(gzl), _dptr_or_null(gzu),
                                _dptr_or_null(gcons)))
    g = Ref(MadipmQPGradients(_dptr_or_null(c), _dptr_or_null(Hvals), _dptr_or_null(Avals), _dptr_or_null(lcon),
                              _dptr_or_null(ucon), _dptr_or_null(lvar), _dptr_or_null(uvar)))
    check(ccall((:madipm_solver_adjoint_polished_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}, Ptr{Cvoid}), h, ct, g, stream),
          "madipm_solver_adjoint_polished_device")
    return
end

# (n_tangents, n_adjoints, n_factorizations, last_residual): successful polished calls, the factorisations that
# restored the polish's factor, the max-norm of the last call's final masked residual
function solver_polished_sens_info(h::Ptr{Cvoid})
    nt, na, nf, r = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Float64}(0.0)
    check(ccall((:madipm_solver_polished_sens_info, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Float64}), h, nt, na, nf, r),
          "madipm_solver_polished_sens_info")
    return (n_tangents = nt[], n_adjoints = na[], n_factorizations = nf[], last_residual = r[])
end

# ---- active-set solve of the data the solver holds, without the interior-point method (ABI 0.2.12).  From a
# starting set (active_var / active_row as in solver_polish; both nothing: the kept set, the codes of the last
# solver_polish or active-set solve that ended polished) up to max_rounds rounds of the polish's factor, solves and
# verdict, the set repaired between them.  It needs no solve: it runs on a fresh solver, after an update, or after
# a solve.  The five blocks are written on verdict 0 only; out_active_var / out_active_row always receive the last
# set tried.  A polished call's point is the one solver_tangent_polished / solver_adjoint_polished differentiate.
struct MadipmActiveSetOpts
    polish::MadipmPolishOpts
    max_rounds::Int32
end
struct MadipmActiveSetInfo
    verdict::Int32
    rounds::Int32
    n_active::Int32
    n_changed::Int32
    residual::Float64
    min_multiplier::Float64
    min_gap::Float64
    n_calls::Int64
    n_factorizations::Int64
end
MadipmActiveSetInfo() = MadipmActiveSetInfo(-1, 0, 0, 0, 0.0, 0.0, 0.0, 0, 0)

function active_set_default_opts()
    o = Ref(MadipmActiveSetOpts(MadipmPolishOpts(0.0, 0.0, 0.0, 0.0, 0), 0))
    ccall((:madipm_active_set_default_opts, libmadipm), Cvoid, (Ref{MadipmActiveSetOpts},), o)
    return o[]
end

# host arrays, as solver_polish
function solver_active_set_solve(h::Ptr{Cvoid}; opts::MadipmActiveSetOpts=active_set_default_opts(),
                                 active_var=nothing, active_row=nothing, x=nothing, y=nothing, zl=nothing,
                                 zu=nothing, cons=nothing, out_active_var=nothing, out_active_row=nothing)
    info = Ref(MadipmActiveSetInfo())
    GC.@preserve active_var active_row x y zl zu cons out_active_var out_active_row begin
        o = Ref(MadipmPolishOut(_ptr_or_null(x), _ptr_or_null(y), _ptr_or_null(zl), _ptr_or_null(zu),
                                _ptr_or_null(cons), _i8ptr_or_null(out_active_var), _i8ptr_or_null(out_active_row)))
        check(ccall((:madipm_solver_active_set_solve, libmadipm), Cint,
                    (Ptr{Cvoid}, Ref{MadipmActiveSetOpts}, Ptr{Int8}, Ptr{Int8}, Ref{MadipmPolishOut},
                     Ref{MadipmActiveSetInfo}),
                    h, Ref(opts), _i8ptr_or_null(active_var), _i8ptr_or_null(active_row), o, info),
              "madipm_solver_active_set_solve")
    end
    return info[]
end

# device arrays and the stream contract of solver_polish_device; the info comes back on the host
function solver_active_set_solve_device(h::Ptr{Cvoid}; opts::MadipmActiveSetOpts=active_set_default_opts(),
                                        active_var=nothing, active_row=nothing, x=nothing, y=nothing, zl=nothing,
                                        zu=nothing, cons=nothing, out_active_var=nothing, out_active_row=nothing,
                                        stream::Ptr{Cvoid}=C_NULL)
    info = Ref(MadipmActiveSetInfo())
    o = Ref(MadipmPolishOut(_dptr_or_null(x), _dptr_or_null(y), _dptr_or_null(zl), _dptr_or_null(zu),
                            _dptr_or_null(cons), _i8ptr_or_null(out_active_var), _i8ptr_or_null(out_active_row)))
    check(ccall((:madipm_solver_active_set_solve_device, libmadipm), Cint,
                (Ptr{Cvoid}, Ref{MadipmActiveSetOpts}, Ptr{Int8}, Ptr{Int8}, Ref{MadipmPolishOut},
                 Ref{MadipmActiveSetInfo}, Ptr{Cvoid}),
                h, Ref(opts), _i8ptr_or_null(active_var), _i8ptr_or_null(active_row), o, info, stream),
          "madipm_solver_active_set_solve_device")
    return info[]
end

function solver_active_set_info(h::Ptr{Cvoid})
    info = Ref(MadipmActiveSetInfo())
    check(ccall((:madipm_solver_active_set_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmActiveSetInfo}), h, info),
          "madipm_solver_active_set_info")
    return info[]
end

# ---- batched sensitivities (ABI 0.2.13): k tangents or adjoints of one point per call.  Every array holds k
# vectors back to back (a k-column Matrix{Float64} in Julia's column-major layout is exactly that); nothing is 0 in
# every column (inputs) or not wanted (outputs).  Column j of every output has the bits of the single call on
# column j.  polished = true differentiates the polished point, one single polished call per column inside the
# library.
sens_batch_cols() = Int(ccall((:madipm_sens_batch_cols, libmadipm), Cint, ()))
_ptr_or_null(a::Matrix{Float64}) = pointer(a)   # len x k: column j is vector j

function solver_tangent_batch(h::Ptr{Cvoid}, k::Integer; dc=nothing, dHvals=nothing, dAvals=nothing, dlcon=nothing,
                              ducon=nothing, dlvar=nothing, duvar=nothing, x=nothing, y=nothing, zl=nothing,
                              zu=nothing, cons=nothing, polished::Bool=false)
    GC.@preserve dc dHvals dAvals dlcon ducon dlvar duvar x y zl zu cons begin
        d = Ref(MadipmQPDirections(_ptr_or_null(dc), _ptr_or_null(dHvals), _ptr_or_null(dAvals), _ptr_or_null(dlcon),
                                   _ptr_or_null(ducon), _ptr_or_null(dlvar), _ptr_or_null(duvar)))
        o = Ref(MadipmQPPointTangents(_ptr_or_null(x), _ptr_or_null(y), _ptr_or_null(zl), _ptr_or_null(zu),
                                      _ptr_or_null(cons)))
        check(ccall((:madipm_solver_tangent_batch, libmadipm), Cint,
                    (Ptr{Cvoid}, Int32, Ref{MadipmQPDirections}, Ref{MadipmQPPointTangents}, Int32),
                    h, k, d, o, polished ? 1 : 0), "madipm_solver_tangent_batch")
    end
    return
end

# DEVICE arrays (Ptr{Float64} into device memory, or nothing), with solver_adjoint_device's stream contract
function solver_tangent_batch_device(h::Ptr{Cvoid}, k::Integer; dc=nothing, dHvals=nothing, dAvals=nothing,
                                     dlcon=nothing, ducon=nothing, dlvar=nothing, duvar=nothing, x=nothing,
                                     y=nothing, zl=nothing, zu=nothing, cons=nothing, polished::Bool=false,
                                     stream::Ptr{Cvoid}=C_NULL)
    d = Ref(MadipmQPDirections(_dptr_or_null(dc), _dptr_or_null(dHvals), _dptr_or_null(dAvals), _dptr_or_null(dlcon),
                               _dptr_or_null(ducon), _dptr_or_null(dlvar), _dptr_or_null(duvar)))
    o = Ref(MadipmQPPointTangents(_dptr_or_null(x), _dptr_or_null(y), _dptr_or_null(zl), _dptr_or_null(zu),
                                  _dptr_or_null(cons)))
    check(ccall((:madipm_solver_tangent_batch_device, libmadipm), Cint,
                (Ptr{Cvoid}, Int32, Ref{MadipmQPDirections}, Ref{MadipmQPPointTangents}, Int32, Ptr{Cvoid}),
                h, k, d, o, polished ? 1 : 0, stream), "madipm_solver_tangent_batch_device")
    return
end

function solver_adjoint_batch(h::Ptr{Cvoid}, k::Integer; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing,
                              gcons=nothing, c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing, ucon=nothing,
                              lvar=nothing, uvar=nothing, polished::Bool=false)
    GC.@preserve gx gy gzl gzu gcons c Hvals Avals lcon ucon lvar uvar begin
        ct = Ref(MadipmQPCotangents(_ptr_or_null(gx), _ptr_or_null(gy), _ptr_or_null(gzl), _ptr_or_null(gzu),
                                    _ptr_or_null(gcons)))
        g = Ref(MadipmQPGradients(_ptr_or_null(c), _ptr_or_null(Hvals), _ptr_or_null(Avals), _ptr_or_null(lcon),
                                  _ptr_or_null(ucon), _ptr_or_null(lvar), _ptr_or_null(uvar)))
        check(ccall((:madipm_solver_adjoint_batch, libmadipm), Cint,
                    (Ptr{Cvoid}, Int32, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}, Int32),
                    h, k, ct, g, polished ? 1 : 0), "madipm_solver_adjoint_batch")
    end
    return
end

function solver_adjoint_batch_device(h::Ptr{Cvoid}, k::Integer; gx=nothing, gy=nothing, gzl=nothing, gzu=nothing,
                                     gcons=nothing, c=nothing, Hvals=nothing, Avals=nothing, lcon=nothing,
                                     ucon=nothing, lvar=nothing, uvar=nothing, polished::Bool=false,
                                     stream::Ptr{Cvoid}=C_NULL)
    ct = Ref(MadipmQPCotangents(_dptr_or_null(gx), _dptr_or_null(gy), _dptr_or_null(gzl), _dptr_or_null(gzu),
                                _dptr_or_null(gcons)))
    g = Ref(MadipmQPGradients(_dptr_or_null(c), _dptr_or_null(Hvals), _dptr_or_null(Avals), _dptr_or_null(lcon),
                              _dptr_or_null(ucon), _dptr_or_null(lvar), _dptr_or_null(uvar)))
    check(ccall((:madipm_solver_adjoint_batch_device, libmadipm), Cint,
                (Ptr{Cvoid}, Int32, Ref{MadipmQPCotangents}, Ref{MadipmQPGradients}, Int32, Ptr{Cvoid}),
                h, k, ct, g, polished ? 1 : 0, stream), "madipm_solver_adjoint_batch_device")
    return
end

# (n_batches, n_columns, n_chunks): successful batched calls, their columns, the chunks of sens_batch_cols() columns
function solver_sens_batch_info(h::Ptr{Cvoid})
    nb, nc, nk = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:madipm_solver_sens_batch_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                h, nb, nc, nk), "madipm_solver_sens_batch_info")
    return (n_batches = nb[], n_columns = nc[], n_chunks = nk[])
end

# ---- multi-right-hand-side LDL^T solve (ABI 0.2.14, DESIGN §13j).  Like every entry of this file these four
# are not executed in this repository (no Julia toolchain in the image): unexercised; the Python mirror
# (HIPLDLSolver.solve_multi / multi_info, MPCSolver.set_multi_solve / multi_solve_info) is the tested one.
# struct madipm_ldl_multi_info
struct MadipmLDLMultiInfo
    width::Int32
    native::Int32
    n_calls::Int64
    n_chunks::Int64
    n_columns::Int64
    n_big_fronts::Int64
end
MadipmLDLMultiInfo() = MadipmLDLMultiInfo(0, 0, 0, 0, 0, 0)

# nrhs columns of length n in place at the DEVICE pointer d_x (column j at d_x + j n): one pass over the factor
# per chunk of `width` columns; a column's bits depend neither on nrhs nor on its position
function ldl_solve_multi(h::Ptr{Cvoid}, d_x::Ptr{Float64}, nrhs::Integer; stream::Ptr{Cvoid}=C_NULL)
    check(ccall((:madipm_ldl_solve_multi, libmadipm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Cvoid}),
                h, d_x, nrhs, stream), "madipm_ldl_solve_multi")
    return
end

function ldl_multi_info(h::Ptr{Cvoid})
    info = Ref(MadipmLDLMultiInfo())
    check(ccall((:madipm_ldl_multi_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmLDLMultiInfo}), h, info),
          "madipm_ldl_multi_info")
    return info[]
end

# on: the batched interior-point sensitivities solve every chunk with the multi-right-hand-side solve
function solver_set_multi_solve(h::Ptr{Cvoid}, on::Bool=true)
    check(ccall((:madipm_solver_set_multi_solve, libmadipm), Cint, (Ptr{Cvoid}, Int32), h, on ? 1 : 0),
          "madipm_solver_set_multi_solve")
    return
end

function solver_multi_solve_info(h::Ptr{Cvoid})
    info = Ref(MadipmLDLMultiInfo())
    check(ccall((:madipm_solver_multi_solve_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmLDLMultiInfo}), h, info),
          "madipm_solver_multi_solve_info")
    return info[]
end

# ---- multi-column big fronts of the multi-right-hand-side solve (ABI 0.2.15, DESIGN §13k); unexercised here
# like the four entries above, whose Python mirror (HIPLDLSolver.set_multi_big / multi_info,
# MPCSolver.multi_solve_info) is the tested one.
# struct madipm_ldl_multi_big_info
struct MadipmLDLMultiBigInfo
    multi_big::Int32
    n_big_levels::Int32
    n_big_passes::Int64
    big_bytes::Int64
end
MadipmLDLMultiBigInfo() = MadipmLDLMultiBigInfo(0, 0, 0, 0)

# on (the default): the big fronts carry a chunk's columns in one pass per level and direction; off: column after
# column with the single-column kernels.  The rows of ldl_solve_multi are bit for bit the same either way.
function ldl_set_multi_big(h::Ptr{Cvoid}, on::Bool=true)
    check(ccall((:madipm_ldl_set_multi_big, libmadipm), Cint, (Ptr{Cvoid}, Int32), h, on ? 1 : 0),
          "madipm_ldl_set_multi_big")
    return
end

function ldl_multi_big_info(h::Ptr{Cvoid})
    info = Ref(MadipmLDLMultiBigInfo())
    check(ccall((:madipm_ldl_multi_big_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmLDLMultiBigInfo}), h, info),
          "madipm_ldl_multi_big_info")
    return info[]
end

function solver_multi_big_info(h::Ptr{Cvoid})
    info = Ref(MadipmLDLMultiBigInfo())
    check(ccall((:madipm_solver_multi_big_info, libmadipm), Cint, (Ptr{Cvoid}, Ref{MadipmLDLMultiBigInfo}), h, info),
          "madipm_solver_multi_big_info")
    return info[]
end
