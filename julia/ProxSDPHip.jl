# ProxSDPHip.jl -- the reference-side binding of libproxsdp_hip.so.
#
# UNTESTED IN THIS REPOSITORY'S ENVIRONMENT: neither the build container nor the GPU box has a
# Julia toolchain (no `julia` binary, no package depot), so this file is shipped as the source a
# ProxSDP maintainer would add.  The C signatures below are exactly include/proxsdp_hip.h; the
# same ABI is exercised by the Python ctypes binding (proxsdp.jl_amd/binding.py), which is what
# the test-suite runs.
#
# How it plugs in.  ProxSDP reaches its solver through ONE call,
#     sol = @timeit "Main" chambolle_pock(aff, con, options)        # src/MOI_wrapper.jl:310
# inside `_optimize!` (src/MOI_wrapper.jl:220-342).  Replace that line by
#     sol = ProxSDPHip.chambolle_pock_hip(aff, con, options)
# and everything above it -- `Optimizer <: MOI.AbstractOptimizer`, copy_to, the attribute
# getters at :362-530, JuMP models -- stays unchanged.  `aff::AffineSets`, `con::ConicSets`,
# `options::Options` and the returned `Result` are the reference's own types
# (src/structs.jl:32-81, src/options.jl).
module ProxSDPHip

import SparseArrays

const libproxsdp_hip = get(ENV, "PROXSDP_HIP_LIB", "libproxsdp_hip.so")

struct CSC                       # proxsdp_csc
    nrows::Int64
    ncols::Int64
    colptr::Ptr{Int64}
    rowval::Ptr{Int64}
    nzval::Ptr{Float64}
end

struct Problem                   # proxsdp_problem
    n::Int64
    p::Int64
    m::Int64
    A::CSC
    G::CSC
    b::Ptr{Float64}
    h::Ptr{Float64}
    c::Ptr{Float64}
    n_psd::Int64
    psd_ptr::Ptr{Int64}
    psd_idx::Ptr{Int64}
    n_soc::Int64
    soc_ptr::Ptr{Int64}
    soc_idx::Ptr{Int64}
    index_base::Int32
    reserved0::Int32
    eig_resid::Ptr{Float64}
    reduce_ctx::Ptr{Cvoid}       # block-sharded solves only (INTEGRATION.md); C_NULL otherwise
    reduce_fn::Ptr{Cvoid}
    M_dense::Ptr{Float64}        # optional dense A (row-major p x n); C_NULL = use the CSC A
    M_dense_on_device::Int32
    reserved1::Int32
    n_coupling::Int64            # coupling rows of a block-sharded solve (0 otherwise)
    coupling_rows::Ptr{Int64}
    coupling_owned::Ptr{Int32}
    reduce_vec_fn::Ptr{Cvoid}
    reduce_vec_on_device::Int32
    reserved2::Int32
    nccl_comm::Ptr{Cvoid}        # RCCL communicator of a block-sharded solve (C_NULL otherwise)
    reserved3::Int64
end

struct Stats                     # proxsdp_stats
    lanczos_matvecs::Int64
    lanczos_restarts::Int64
    lanczos_calls::Int64
    full_eigs::Int64
    krylov_fallbacks::Int64
    linesearch_trials::Int64
    symv_launches::Int64
    symv_profiled::Int64
    symv_profiled_ms::Float64
    symv_bytes::Float64
    algorithmic_bytes::Float64
    init_time::Float64
    loop_time::Float64
    exit_time::Float64
    t_primal::Float64
    t_psd::Float64
    t_linesearch::Float64
    t_residual::Float64
    dense_passes::Int64
    dense_ms::Float64
    fop_projections::Int64
    exit_matvecs::Int64
    host_eig_time::Float64
    host_eigs::Int64
    device_eigs::Int64
    batched_small_eigs::Int64
    mfma_reconstructions::Int64
    orth_profiled::Int64
    orth_profiled_ms::Float64
    full_eig_solver_ms::Float64
    full_eig_recon_ms::Float64
    cycle_launches::Int64
    full_eigs_lanczos::Int64
    cycle_steps::Int64
    cycle_ms::Float64
    warm_starts::Int64
    full_eigs_sign::Int64
    sign_products::Int64
    sign_engine_projections::Int64
    sign_engine_rejected::Int64
    sign_engine_checks::Int64
    sign_engine_mismatches::Int64
    full_eigs_lanczos_checks::Int64
    full_eigs_lanczos_mismatches::Int64
    batched_block_steps::Int64
    rccl_reductions::Int64
    batched_profiled_blocks::Int64
    host_eig_merges::Int64
    host_eig_overlap_time::Float64
    sign_short_pass::Int64
    sign_short_fail::Int64
    full_eigs_lanczos_certified::Int64
    full_eigs_lanczos_cert_failed::Int64
    cert_matvecs::Int64
    dense_truncated_projections::Int64
    wide_krylov_projections::Int64
    reserved_s::NTuple{4,Int64}
    dense_setup_passes::Int64
    dense_sigma_steps::Int64
end
# named slots of Stats.reserved_s (PROXSDP_STATS_* in the header, 0-based there): iterations a block-sharded solve ran on
# the general vector path on this shard
sharded_general_iterations(s::Stats) = s.reserved_s[1]
# merges of host_eig_merges whose O(k^2) part ran on the device (option device_eig_merge), and merges the host did while
# that path was switched on
device_eig_merges(s::Stats) = s.reserved_s[2]
device_eig_merge_fallbacks(s::Stats) = s.reserved_s[3]
# k_lz_orth launches of the operator-form Lanczos step on the owner form (t = Vp'v finished in the mat-vec launch)
fop_owner_steps(s::Stats) = s.reserved_s[4]

mutable struct CResult           # proxsdp_result
    status::Int32
    certificate_found::Int32
    primal_feasible_user_tol::Int32
    dual_feasible_user_tol::Int32
    result_count::Int32
    final_rank::Int32
    iter::Int64
    primal_residual::Float64
    dual_residual::Float64
    objval::Float64
    dual_objval::Float64
    gap::Float64
    time::Float64
    dual_feasibility::Float64
    primal::Ptr{Float64}
    dual_cone::Ptr{Float64}
    dual_eq::Ptr{Float64}
    dual_in::Ptr{Float64}
    slack_eq::Ptr{Float64}
    slack_in::Ptr{Float64}
    trace::Ptr{Float64}
    trace_rows::Int64
    status_string::NTuple{256,UInt8}
    stats::Stats
    CResult() = new()
end

struct PsdFactors                # proxsdp_psd_factors
    struct_size::Int64
    n_psd::Int64
    cap::Ptr{Int64}
    vec_ptr::Ptr{Int64}
    val_ptr::Ptr{Int64}
    vectors::Ptr{Float64}
    values::Ptr{Float64}
    rank::Ptr{Int64}
    rank_found::Ptr{Int64}
    source::Ptr{Int32}
    resid::Ptr{Float64}
    xnorm::Ptr{Float64}
end
const FACTOR_NONE = Int32(0); const FACTOR_RITZ = Int32(1); const FACTOR_EIG = Int32(2)   # PROXSDP_FACTOR_*

struct Start                     # proxsdp_start
    struct_size::Int64
    primal::Ptr{Float64}
    dual_eq::Ptr{Float64}
    dual_in::Ptr{Float64}
    n_psd::Int64
    rank::Ptr{Int64}
    vec_ptr::Ptr{Int64}
    val_ptr::Ptr{Int64}
    vectors::Ptr{Float64}
    values::Ptr{Float64}
    target_rank::Ptr{Int64}
    primal_step::Float64
    beta::Float64
end

struct DeviceVectors             # proxsdp_device_vectors: DEVICE pointers, borrowed and trusted (C_NULL = not wanted / not given)
    struct_size::Int64
    device_id::Int32
    reserved::Int32
    primal::Ptr{Float64}
    dual_cone::Ptr{Float64}
    dual_eq::Ptr{Float64}
    slack_eq::Ptr{Float64}
    dual_in::Ptr{Float64}
    slack_in::Ptr{Float64}
end
function _device_vectors(nt::NamedTuple)
    g(name) = haskey(nt, name) ? Ptr{Float64}(getfield(nt, name)) : Ptr{Float64}(C_NULL)
    DeviceVectors(sizeof(DeviceVectors), Int32(haskey(nt, :device_id) ? nt.device_id : 0), Int32(0),
                  g(:primal), g(:dual_cone), g(:dual_eq), g(:slack_eq), g(:dual_in), g(:slack_in))
end

# proxsdp_options is filled by name, exactly like MOI.RawOptimizerAttribute does for the
# reference (src/MOI_wrapper.jl:84-93): an opaque, suitably large and aligned buffer plus
# proxsdp_hip_default_options / proxsdp_hip_set_option keeps this file independent of the C
# struct layout.
const OPTIONS_BYTES = 1024

function _options_buffer(options)
    buf = zeros(UInt64, OPTIONS_BYTES ÷ 8)
    ccall((:proxsdp_hip_default_options, libproxsdp_hip), Cvoid, (Ptr{UInt64},), buf)
    for name in fieldnames(typeof(options))
        v = getfield(options, name)
        v isa Union{Bool,Integer,AbstractFloat} || continue
        rc = ccall((:proxsdp_hip_set_option, libproxsdp_hip), Cint,
                   (Ptr{UInt64}, Cstring, Cdouble), buf, String(name), Float64(v))
        rc == 0 || error("No parameter matching $(name)")   # same text as MOI_wrapper.jl:90
    end
    return buf
end

_csc(M::SparseArrays.SparseMatrixCSC{Float64,Int64}) =
    CSC(size(M, 1), size(M, 2), pointer(M.colptr), pointer(M.rowval), pointer(M.nzval))

"""
    chambolle_pock_hip(aff, con, options) -> Result

Drop-in for `chambolle_pock(aff, con, options)` (src/pdhg.jl:1-530).  `aff`/`con` are only read;
the library works on private copies (the reference mutates `aff`: src/scaling.jl:24,
src/pdhg.jl:647-663).

`n_shards > 1` (or `device_ids` given): the block-sharded solve from this one call (`proxsdp_hip_solve_sharded`) -- the
library splits the model over `n_shards` shards, runs them as host threads of this process, shard `s` on device
`device_ids[s]` (0-based HIP ordinals; default: all on the device the options name), and returns the whole model's
result in the caller's order.  Cones are dealt out round-robin (PSD cones, then SOC cones, then the free variables).

`factors = true` or a vector of column caps, one per PSD cone (0 = none for that cone): the same solve through
`proxsdp_hip_solve_factored`; the return value is then `(result, factors)` with `factors[k] = (values, vectors, info)`,
`X_k ≈ vectors * Diagonal(values) * vectors'`, values descending and positive, `info = (rank, rank_found, source, resid,
xnorm)` -- what a caller of the reference computes with `eigen` on the returned block.  Not with `n_shards > 1`.
`start = (primal = ..., dual_eq = ..., dual_in = ..., factors = ..., target_rank = ..., primal_step = ..., beta = ...)`
(a NamedTuple, every field optional): a warm start through `proxsdp_hip_solve_from`.  `primal`, `dual_eq`, `dual_in` are
what a previous `Result` holds; `factors[k] = (values, vectors)` or `nothing` per PSD cone (the factors a previous
`factors = true` solve returned: that cone then starts at `vectors * Diagonal(values) * vectors'` and at target rank
`length(values) + 1`); `target_rank[k] > 0` overrides the target rank of cone k.  Combines with `factors`, not with
`n_shards > 1`.
`device_out = (device_id = 0, primal = ptr, dual_cone = ptr, dual_eq = ptr, slack_eq = ptr, dual_in = ptr, slack_in = ptr)`
and / or `start_dev = (device_id = 0, primal = ptr, dual_eq = ptr, dual_in = ptr)` (NamedTuples of DEVICE pointers, e.g.
`pointer(::ROCArray{Float64})`; every field optional): the solve through `proxsdp_hip_solve_device`.  The six vectors of
the result are written into the caller's device buffers, in the caller's order and in the units of a `Result` (the host
vectors of the returned `Result` receive the same values), and the start point's `primal`, `dual_eq`, `dual_in` are read
from device buffers in those same units (a vector may be given in `start` or in `start_dev`, not both; factors, target
ranks and steps stay in `start`).  `device_id` must be the device the options name.  The pointers are borrowed and
trusted, as a device `M_dense` is; the library runs on its own stream, so synchronise the device before the call -- it
returns after its writes have completed.  Not with `n_shards > 1`.  (Like the rest of this wrapper the two keywords cannot
be run where the library is tested; the struct is checked against the header, the entry through the ctypes binding.)
(This wrapper cannot be executed where the library is tested: there is no Julia there.  Its struct is checked against the
header field by field, the call itself is exercised through the ctypes binding.)
"""
function chambolle_pock_hip(aff, con, options; ResultType = Main.ProxSDP.Result,
                            n_shards::Integer = 1, device_ids::Union{Nothing,AbstractVector{<:Integer}} = nothing,
                            factors::Union{Nothing,Bool,AbstractVector{<:Integer}} = nothing,
                            start::Union{Nothing,NamedTuple} = nothing,
                            device_out::Union{Nothing,NamedTuple} = nothing,
                            start_dev::Union{Nothing,NamedTuple} = nothing)
    psd_ptr = Int64[0]; psd_idx = Int64[]
    for s in con.sdpcone
        append!(psd_idx, s.vec_i); push!(psd_ptr, length(psd_idx))
    end
    soc_ptr = Int64[0]; soc_idx = Int64[]
    for s in con.socone
        append!(soc_idx, s.idx); push!(soc_ptr, length(soc_idx))
    end
    n, p, m = aff.n, aff.p, aff.m
    primal = zeros(n); dual_cone = zeros(n)
    dual_eq = zeros(p); dual_in = zeros(m); slack_eq = zeros(p); slack_in = zeros(m)
    opt = _options_buffer(options)
    res = CResult()
    A, G = aff.A, aff.G
    sharded = n_shards > 1 || device_ids !== nothing
    devs = device_ids === nothing ? Int32[] : Int32.(device_ids)
    (device_ids === nothing || length(devs) == n_shards) || error("device_ids: one device per shard")
    want_factors = factors !== nothing && factors !== false
    (want_factors && sharded) && error("factors: not available in a block-sharded solve")
    nb = length(con.sdpcone)
    sides = Int64[s.sq_side for s in con.sdpcone]
    caps = !want_factors ? zeros(Int64, nb) : factors === true ? copy(sides) : min.(Int64.(factors), sides)
    length(caps) == nb || error("factors: one cap per PSD cone")
    fvec_ptr = Int64[0]; fval_ptr = Int64[0]
    for k in 1:nb
        push!(fvec_ptr, fvec_ptr[end] + sides[k] * caps[k]); push!(fval_ptr, fval_ptr[end] + caps[k])
    end
    fvectors = zeros(max(fvec_ptr[end], 1)); fvalues = zeros(max(fval_ptr[end], 1))
    frank = zeros(Int64, max(nb, 1)); ffound = zeros(Int64, max(nb, 1)); fsource = zeros(Int32, max(nb, 1))
    fresid = zeros(max(nb, 1)); fxnorm = zeros(max(nb, 1))
    # warm start: the caller's arrays as Float64 / Int64 vectors, the factors of every cone concatenated column-major
    (start !== nothing && sharded) && error("start: not available in a block-sharded solve")
    on_device = device_out !== nothing || start_dev !== nothing
    (on_device && sharded) && error("device_out / start_dev: not available in a block-sharded solve")
    sget(name) = (start !== nothing && haskey(start, name)) ? getfield(start, name) : nothing
    s_primal = sget(:primal) === nothing ? Float64[] : Vector{Float64}(sget(:primal))
    s_deq = sget(:dual_eq) === nothing ? Float64[] : Vector{Float64}(sget(:dual_eq))
    s_din = sget(:dual_in) === nothing ? Float64[] : Vector{Float64}(sget(:dual_in))
    (sget(:primal) === nothing || length(s_primal) == n) || error("start.primal: length n")
    (sget(:dual_eq) === nothing || length(s_deq) == p) || error("start.dual_eq: length p")
    (sget(:dual_in) === nothing || length(s_din) == m) || error("start.dual_in: length m")
    s_fac = sget(:factors)
    s_rank = fill(Int64(-1), max(nb, 1)); s_vec_ptr = Int64[0]; s_val_ptr = Int64[0]
    s_vectors = Float64[]; s_values = Float64[]
    if s_fac !== nothing
        length(s_fac) == nb || error("start.factors: one entry per PSD cone")
        for k in 1:nb
            if s_fac[k] !== nothing
                vals = Vector{Float64}(s_fac[k][1]); V = Matrix{Float64}(s_fac[k][2])
                size(V) == (sides[k], length(vals)) || error("start.factors[$k]: vectors must be side x rank")
                s_rank[k] = length(vals); append!(s_vectors, vec(V)); append!(s_values, vals)
            end
            push!(s_vec_ptr, length(s_vectors)); push!(s_val_ptr, length(s_values))
        end
    end
    push!(s_vectors, 0.0); push!(s_values, 0.0)                          # (never empty: a valid pointer)
    s_tr = sget(:target_rank) === nothing ? Int64[] : Vector{Int64}(sget(:target_rank))
    (sget(:target_rank) === nothing || length(s_tr) == nb) || error("start.target_rank: one entry per PSD cone")
    ptr_or_null(v, given) = given ? pointer(v) : Ptr{eltype(v)}(C_NULL)
    GC.@preserve A G aff psd_ptr psd_idx soc_ptr soc_idx primal dual_cone dual_eq dual_in slack_eq slack_in opt devs caps fvec_ptr fval_ptr fvectors fvalues frank ffound fsource fresid fxnorm s_primal s_deq s_din s_rank s_vec_ptr s_val_ptr s_vectors s_values s_tr begin
        prob = Problem(n, p, m, _csc(A), _csc(G), pointer(aff.b), pointer(aff.h), pointer(aff.c),
                       length(con.sdpcone), pointer(psd_ptr), pointer(psd_idx),
                       length(con.socone), pointer(soc_ptr), pointer(soc_idx),
                       Int32(1), Int32(0), Ptr{Float64}(C_NULL),         # Julia indices are 1-based
                       C_NULL, C_NULL, Ptr{Float64}(C_NULL), Int32(0), Int32(0),
                       0, Ptr{Int64}(C_NULL), Ptr{Int32}(C_NULL), C_NULL, Int32(0), Int32(0),   # no coupling rows
                       C_NULL, 0)                                                                # no RCCL communicator
        res.primal = pointer(primal); res.dual_cone = pointer(dual_cone)
        res.dual_eq = pointer(dual_eq); res.dual_in = pointer(dual_in)
        res.slack_eq = pointer(slack_eq); res.slack_in = pointer(slack_in)
        res.trace = Ptr{Float64}(C_NULL); res.trace_rows = 0
        rc = if sharded
            ccall((:proxsdp_hip_solve_sharded, libproxsdp_hip), Cint,
                  (Ref{Problem}, Ptr{UInt64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ref{CResult}, Ptr{Stats}),
                  prob, opt, Int32(n_shards), device_ids === nothing ? Ptr{Int32}(C_NULL) : pointer(devs),
                  C_NULL, C_NULL, C_NULL, res, C_NULL)                # default owners, no per-shard stats
        elseif on_device
            st = Start(sizeof(Start), ptr_or_null(s_primal, sget(:primal) !== nothing),
                       ptr_or_null(s_deq, sget(:dual_eq) !== nothing && p > 0), ptr_or_null(s_din, sget(:dual_in) !== nothing && m > 0),
                       s_fac === nothing ? 0 : nb, pointer(s_rank), pointer(s_vec_ptr), pointer(s_val_ptr),
                       pointer(s_vectors), pointer(s_values), ptr_or_null(s_tr, sget(:target_rank) !== nothing && nb > 0),
                       sget(:primal_step) === nothing ? 0.0 : Float64(sget(:primal_step)),
                       sget(:beta) === nothing ? 0.0 : Float64(sget(:beta)))
            fac = PsdFactors(sizeof(PsdFactors), nb, pointer(caps), pointer(fvec_ptr), pointer(fval_ptr),
                             pointer(fvectors), pointer(fvalues), pointer(frank), pointer(ffound), pointer(fsource),
                             pointer(fresid), pointer(fxnorm))
            sdv = start_dev === nothing ? nothing : _device_vectors(start_dev)
            odv = device_out === nothing ? nothing : _device_vectors(device_out)
            ccall((:proxsdp_hip_solve_device, libproxsdp_hip), Cint,
                  (Ref{Problem}, Ptr{UInt64}, Ref{CResult}, Ptr{Start}, Ptr{DeviceVectors}, Ptr{PsdFactors}, Ptr{DeviceVectors}),
                  prob, opt, res, start === nothing ? C_NULL : Ref(st), sdv === nothing ? C_NULL : Ref(sdv),
                  want_factors ? Ref(fac) : C_NULL, odv === nothing ? C_NULL : Ref(odv))
        elseif start !== nothing
            st = Start(sizeof(Start), ptr_or_null(s_primal, sget(:primal) !== nothing),
                       ptr_or_null(s_deq, sget(:dual_eq) !== nothing && p > 0), ptr_or_null(s_din, sget(:dual_in) !== nothing && m > 0),
                       s_fac === nothing ? 0 : nb, pointer(s_rank), pointer(s_vec_ptr), pointer(s_val_ptr),
                       pointer(s_vectors), pointer(s_values), ptr_or_null(s_tr, sget(:target_rank) !== nothing && nb > 0),
                       sget(:primal_step) === nothing ? 0.0 : Float64(sget(:primal_step)),
                       sget(:beta) === nothing ? 0.0 : Float64(sget(:beta)))
            if want_factors
                fac = PsdFactors(sizeof(PsdFactors), nb, pointer(caps), pointer(fvec_ptr), pointer(fval_ptr),
                                 pointer(fvectors), pointer(fvalues), pointer(frank), pointer(ffound), pointer(fsource),
                                 pointer(fresid), pointer(fxnorm))
                ccall((:proxsdp_hip_solve_from, libproxsdp_hip), Cint,
                      (Ref{Problem}, Ptr{UInt64}, Ref{CResult}, Ref{Start}, Ref{PsdFactors}), prob, opt, res, st, fac)
            else
                ccall((:proxsdp_hip_solve_from, libproxsdp_hip), Cint,
                      (Ref{Problem}, Ptr{UInt64}, Ref{CResult}, Ref{Start}, Ptr{Cvoid}), prob, opt, res, st, C_NULL)
            end
        elseif want_factors
            fac = PsdFactors(sizeof(PsdFactors), nb, pointer(caps), pointer(fvec_ptr), pointer(fval_ptr),
                             pointer(fvectors), pointer(fvalues), pointer(frank), pointer(ffound), pointer(fsource),
                             pointer(fresid), pointer(fxnorm))
            ccall((:proxsdp_hip_solve_factored, libproxsdp_hip), Cint,
                  (Ref{Problem}, Ptr{UInt64}, Ref{CResult}, Ref{PsdFactors}), prob, opt, res, fac)
        else
            ccall((:proxsdp_hip_solve, libproxsdp_hip), Cint,
                  (Ref{Problem}, Ptr{UInt64}, Ref{CResult}), prob, opt, res)
        end
        if rc != 0
            msg = unsafe_string(ccall((:proxsdp_hip_last_error, libproxsdp_hip), Cstring, ()))
            error("libproxsdp_hip: error $(rc): $(msg)")
        end
    end
    status_string = String(UInt8[c for c in res.status_string if c != 0x00])
    result = ResultType(
        res.status, status_string, primal, dual_cone, dual_eq, dual_in, slack_eq, slack_in,
        res.primal_residual, res.dual_residual, res.objval, res.dual_objval, res.gap, res.time,
        res.iter, res.final_rank, res.primal_feasible_user_tol != 0,
        res.dual_feasible_user_tol != 0, res.certificate_found != 0, res.result_count)
    want_factors || return result
    out = [(fvalues[fval_ptr[k]+1:fval_ptr[k]+frank[k]],
            reshape(fvectors[fvec_ptr[k]+1:fvec_ptr[k]+sides[k]*frank[k]], Int(sides[k]), Int(frank[k])),
            (rank = frank[k], rank_found = ffound[k], source = fsource[k], resid = fresid[k], xnorm = fxnorm[k]))
           for k in 1:nb]
    return result, out
end

# ---- separation on a kept model (include/proxsdp_hip.h, "separation on a model handle").  `mdl` is the opaque handle of
# proxsdp_hip_model_create as a Ptr{Cvoid}.  (Like the rest of this file these cannot be executed where the library is tested;
# the structs are checked against the header field by field, the entries through the ctypes binding.)
mutable struct TriangleCuts      # proxsdp_triangle_cuts
    struct_size::Int64
    on_device::Int32
    cone::Int32
    count::Int64
    min_violation::Float64
    rhs::Float64
    cand_cap::Int64
    primal::Ptr{Float64}
    tri::Ptr{Int64}
    pattern::Ptr{Int32}
    violation::Ptr{Float64}
    add_col::Ptr{Int64}
    add_val::Ptr{Float64}
    add_h::Ptr{Float64}
    n_rows::Int64
    violated::Int64
    scanned::Int64
    passes::Int32
    reserved::Int32
    bytes_allocated::Int64
    seconds::Float64
    sweep_seconds::Float64
end

mutable struct InactiveRows      # proxsdp_inactive_rows
    struct_size::Int64
    on_device::Int32
    reserved::Int32
    dual_in::Ptr{Float64}
    slack_in::Ptr{Float64}
    dual_tol::Float64
    slack_tol::Float64
    rows::Ptr{Int64}
    n_rows::Int64
end

function _check_rc(rc)
    rc == 0 && return
    msg = unsafe_string(ccall((:proxsdp_hip_last_error, libproxsdp_hip), Cstring, ()))
    error("libproxsdp_hip: error $(rc): $(msg)")
end

function _triangle_result(tc::TriangleCuts, tri, pattern, violation, add_col, add_val, add_h)
    k = Int(tc.n_rows)
    (triples = permutedims(reshape(tri[1:3k], 3, k)), patterns = pattern[1:k], violations = violation[1:k],
     add_ptr = collect(Int64(0):Int64(3):Int64(3k)), add_col = add_col[1:3k], add_val = add_val[1:3k], add_h = add_h[1:k],
     violated = tc.violated, scanned = tc.scanned, passes = tc.passes, seconds = tc.seconds)
end

"""
    model_triangles(mdl, primal; cone = 1, count = 1000, min_violation = 1e-3, rhs = 1.0, cand_cap = 0, on_device = false)

The `count` most violated triangle inequalities of PSD cone `cone` (1-based here, in cone order) of the kept model `mdl` at
`primal`: a `Vector{Float64}` of n entries, or with `on_device = true` a DEVICE pointer (`Ptr{Float64}`) on the model's
device.  Returns a NamedTuple; `triples` are 0-based `i < j < k` as the library reports them, `add_ptr` / `add_col` /
`add_val` / `add_h` are a `proxsdp_model_rows` change as they stand (`add_col` in the index base of create: 1-based for a
model created from Julia data).
"""
function model_triangles(mdl::Ptr{Cvoid}, primal; cone::Integer = 1, count::Integer = 1000, min_violation::Real = 1e-3,
                         rhs::Real = 1.0, cand_cap::Integer = 0, on_device::Bool = false)
    tri = zeros(Int64, 3count); pattern = zeros(Int32, count); violation = zeros(count)
    add_col = zeros(Int64, 3count); add_val = zeros(3count); add_h = zeros(count)
    GC.@preserve primal tri pattern violation add_col add_val add_h begin
        tc = TriangleCuts(sizeof(TriangleCuts), Int32(on_device), Int32(cone - 1), count, min_violation, rhs, cand_cap,
                          on_device ? Ptr{Float64}(primal) : pointer(primal), pointer(tri), pointer(pattern), pointer(violation),
                          pointer(add_col), pointer(add_val), pointer(add_h), 0, 0, 0, Int32(0), Int32(0), 0, 0.0, 0.0)
        _check_rc(ccall((:proxsdp_hip_model_triangles, libproxsdp_hip), Cint, (Ptr{Cvoid}, Ref{TriangleCuts}), mdl, tc))
    end
    return _triangle_result(tc, tri, pattern, violation, add_col, add_val, add_h)
end

"""
    host_triangle_cuts(X; count = 1000, min_violation = 1e-3, rhs = 1.0, cone_idx = nothing, index_base = 1)

The same separation on the host, serially, for a symmetric `Matrix{Float64}` (no device, no handle).  `cone_idx`: the cone's
variable list (upper triangle column by column, `SDPSet.vec_i`) as `add_col` shall report it; `nothing`: the position in that
list plus `index_base`.
"""
function host_triangle_cuts(X::Matrix{Float64}; count::Integer = 1000, min_violation::Real = 1e-3, rhs::Real = 1.0,
                            cone_idx::Union{Nothing,Vector{Int64}} = nothing, index_base::Integer = 1)
    side = size(X, 1)
    size(X, 2) == side || error("X must be square")
    tri = zeros(Int64, 3count); pattern = zeros(Int32, count); violation = zeros(count)
    add_col = zeros(Int64, 3count); add_val = zeros(3count); add_h = zeros(count)
    GC.@preserve X cone_idx tri pattern violation add_col add_val add_h begin
        tc = TriangleCuts(sizeof(TriangleCuts), Int32(0), Int32(0), count, min_violation, rhs, 0, Ptr{Float64}(C_NULL),
                          pointer(tri), pointer(pattern), pointer(violation), pointer(add_col), pointer(add_val), pointer(add_h),
                          0, 0, 0, Int32(0), Int32(0), 0, 0.0, 0.0)
        # (a symmetric matrix is its own transpose: Julia's column-major storage is the row-major X the entry reads)
        _check_rc(ccall((:proxsdp_host_triangle_cuts, libproxsdp_hip), Cint,
                        (Ptr{Float64}, Int64, Ptr{Int64}, Int32, Ref{TriangleCuts}),
                        X, side, cone_idx === nothing ? Ptr{Int64}(C_NULL) : pointer(cone_idx), Int32(index_base), tc))
    end
    return _triangle_result(tc, tri, pattern, violation, add_col, add_val, add_h)
end

"""
    model_inactive_rows(mdl, dual_in, slack_in, m; dual_tol = 0.0, slack_tol = 1e-6, on_device = false)

The inequality rows of the kept model `mdl` (m of them) with `|dual_in[r]| <= dual_tol` and `slack_in[r] < -slack_tol`, as
ascending 0-BASED numbers: the `drop` list of `proxsdp_hip_model_rows`.  `dual_in` / `slack_in`: `Vector{Float64}`s of a
`Result`, or with `on_device = true` DEVICE pointers.  A NaN row is not inactive.
"""
function model_inactive_rows(mdl::Ptr{Cvoid}, dual_in, slack_in, m::Integer; dual_tol::Real = 0.0, slack_tol::Real = 1e-6,
                             on_device::Bool = false)
    rows = zeros(Int64, max(m, 1))
    GC.@preserve dual_in slack_in rows begin
        q = InactiveRows(sizeof(InactiveRows), Int32(on_device), Int32(0),
                         on_device ? Ptr{Float64}(dual_in) : pointer(dual_in), on_device ? Ptr{Float64}(slack_in) : pointer(slack_in),
                         dual_tol, slack_tol, pointer(rows), 0)
        _check_rc(ccall((:proxsdp_hip_model_inactive_rows, libproxsdp_hip), Cint, (Ptr{Cvoid}, Ref{InactiveRows}), mdl, q))
    end
    return rows[1:Int(q.n_rows)]
end

# ---- a +-1 vector from a kept model's factors (include/proxsdp_hip.h, "rounding on a model handle")
mutable struct Rounding          # proxsdp_rounding
    struct_size::Int64
    on_device::Int32
    cone::Int32
    r::Int32
    trials::Int32
    seed::Int64
    max_sweeps::Int32
    grid_adjacency::Int32
    grid_directions::Int32
    grid_signs::Int32
    grid_search::Int32
    lds_side::Int32
    V::Ptr{Float64}
    values::Ptr{Float64}
    signs::Ptr{Int8}
    values_rounded::Ptr{Float64}
    values_final::Ptr{Float64}
    adj_ptr::Ptr{Int64}
    adj_col::Ptr{Int64}
    adj_val::Ptr{Float64}
    diag::Ptr{Float64}
    adj_cap::Int64
    adj_nnz::Int64
    best_trial::Int64
    value::Float64
    value_rounded::Float64
    flips::Int64
    sweeps::Int32
    reserved::Int32
    bytes_allocated::Int64
    seconds::Float64
    search_seconds::Float64
end

"""
    model_round(mdl, values, V, side; cone = 1, trials = 1024, seed = 0, max_sweeps = 50, on_device = false)

Randomised hyperplane rounding of the factors `V` (`side x r`, a `Matrix{Float64}`: Julia's column-major storage is what the
entry reads) and `values` (`r`, all > 0) of PSD cone `cone` (1-based here) of the kept model `mdl` to `trials` +-1 vectors, each
improved by a one-flip local search against the model's current objective; with `on_device = true` both are DEVICE pointers
and `r = length` must be given as `r`.  Returns a NamedTuple: `signs` (`Vector{Int8}`), `value` (minimisation form),
`value_rounded`, `best_trial` (0-based), `sweeps`, `flips`, `values_rounded`, `values_final`, `seconds`.
"""
function model_round(mdl::Ptr{Cvoid}, values, V, side::Integer; cone::Integer = 1, trials::Integer = 1024, seed::Integer = 0,
                     max_sweeps::Integer = 50, on_device::Bool = false, r::Integer = on_device ? 0 : length(values))
    signs = zeros(Int8, side); vr = zeros(trials); vf = zeros(trials)
    GC.@preserve values V signs vr vf begin
        q = Rounding(sizeof(Rounding), Int32(on_device), Int32(cone - 1), Int32(r), Int32(trials), Int64(seed), Int32(max_sweeps),
                     Int32(0), Int32(0), Int32(0), Int32(0), Int32(0),
                     on_device ? Ptr{Float64}(V) : pointer(V), on_device ? Ptr{Float64}(values) : pointer(values),
                     pointer(signs), pointer(vr), pointer(vf), Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL), Ptr{Float64}(C_NULL),
                     Ptr{Float64}(C_NULL), 0, 0, 0, 0.0, 0.0, 0, Int32(0), Int32(0), 0, 0.0, 0.0)
        _check_rc(ccall((:proxsdp_hip_model_round, libproxsdp_hip), Cint, (Ptr{Cvoid}, Ref{Rounding}), mdl, q))
    end
    return (signs = signs, value = q.value, value_rounded = q.value_rounded, best_trial = q.best_trial, sweeps = q.sweeps,
            flips = q.flips, values_rounded = vr, values_final = vf, seconds = q.seconds)
end

# ---- a certified dual bound of a kept model (include/proxsdp_hip.h, "a certified dual bound of a model handle")
mutable struct DualBound         # proxsdp_dual_bound
    struct_size::Int64
    on_device::Int32
    reserved::Int32
    dual_eq::Ptr{Float64}
    dual_in::Ptr{Float64}
    trace_cap::Ptr{Float64}
    shift::Ptr{Float64}
    lambda_lower::Ptr{Float64}
    radius::Ptr{Float64}
    factorisations::Ptr{Int32}
    certified::Ptr{Int32}
    delta::Ptr{Float64}
    trace_used::Ptr{Float64}
    bound::Float64
    dual_objective::Float64
    bytes_allocated::Int64
    seconds::Float64
    factor_seconds::Float64
end

"""
    model_bound(mdl, dual_eq, dual_in, n_psd; trace_cap = nothing, on_device = false)

A certified LOWER bound of the optimum of the kept model `mdl` (minimisation form: a MAX model's bound is `-bound`, an upper
bound) from any dual point: `dual_eq` / `dual_in` are `Vector{Float64}`s of a `Result`, or with `on_device = true` DEVICE
pointers.  The proof is a completed fp64 Cholesky factorisation on the device with its backward-error bound; no eigenvalue
estimate enters.  `trace_cap`: one number per PSD cone with `tr X_k <= cap` for every feasible x, or `nothing` = derived from
equality rows `a X_ii = b`.  Returns a NamedTuple: `bound` (`-Inf` when a cone could not be certified), `dual_objective`, and
per cone `shift`, `lambda_lower`, `radius`, `delta`, `trace`, `factorisations`, `certified`; `seconds`, `factor_seconds`.
"""
function model_bound(mdl::Ptr{Cvoid}, dual_eq, dual_in, n_psd::Integer; trace_cap = nothing, on_device::Bool = false)
    k = max(n_psd, 1)
    shift = zeros(k); lower = zeros(k); radius = zeros(k); delta = zeros(k); trace = zeros(k)
    tries = zeros(Int32, k); cert = zeros(Int32, k)
    cap = trace_cap === nothing ? Float64[] : Vector{Float64}(trace_cap)
    hostptr(v) = (v === nothing || length(v) == 0) ? Ptr{Float64}(C_NULL) : pointer(v)
    GC.@preserve dual_eq dual_in cap shift lower radius delta trace tries cert begin
        q = DualBound(sizeof(DualBound), Int32(on_device), Int32(0),
                      on_device ? Ptr{Float64}(dual_eq) : hostptr(dual_eq), on_device ? Ptr{Float64}(dual_in) : hostptr(dual_in),
                      hostptr(cap), pointer(shift), pointer(lower), pointer(radius), pointer(tries), pointer(cert), pointer(delta),
                      pointer(trace), 0.0, 0.0, 0, 0.0, 0.0)
        _check_rc(ccall((:proxsdp_hip_model_bound, libproxsdp_hip), Cint, (Ptr{Cvoid}, Ref{DualBound}), mdl, q))
    end
    return (bound = q.bound, dual_objective = q.dual_objective, shift = shift, lambda_lower = lower, radius = radius, delta = delta,
            trace = trace, factorisations = tries, certified = cert .!= 0, seconds = q.seconds, factor_seconds = q.factor_seconds)
end

end # module
