"""Block-sharded solve: one process per GPU, GPU g owns the cones assigned to it -- PSD blocks of any side,
second-order cones -- the variables outside every cone assigned to it, and the constraint rows that touch only its
variables.  The reference processes the blocks of a model serially on one core
(/root/reference/src/prox_operators.jl:40); here every shard runs the full PDHG loop on
its own cones and the shards exchange only scalars (linesearch norms, residual maxima,
objective sums, convergence flags, one clock) through one small collective per
iteration, plus -- when the model has rows that couple variables of different shards -- one
all-reduce of the coupling rows of M x -- `torch.distributed` with backend "nccl" (= RCCL over xGMI) on the GPU box,
"gloo" in the CPU-side tests.  All shards therefore take identical control-flow decisions
and the iterates are those of the single-process solve of the whole model.  A shard whose cones are PSD blocks of
side >= 2 only runs the library's support-aware vector path, any other shard the general one; `gather_solution`
puts the shards' results back into the caller's variable and row order.
"""
import numpy as np
import scipy.sparse as sp

from . import problems
from .optimizer import Optimizer


def free_variables(prob):
    """ids of the variables outside every cone, ascending"""
    free = np.ones(prob.n, dtype=bool)
    for idx in list(prob.psd) + list(prob.soc):
        free[np.asarray(idx, dtype=np.int64)] = False
    return np.nonzero(free)[0]


def default_owners(prob, world):
    """(owners, soc_owners, free_owners): one round-robin over the PSD cones, then the SOC cones, then the free variables
    in ascending id -- a pure function of the model and `world`, so every rank computes the same map.  Any other
    assignment is as correct (a cone is never split; a poor one only makes more rows coupling rows)."""
    n_psd, n_soc, n_free = len(prob.psd), len(prob.soc), len(free_variables(prob))
    rr = lambda start, cnt: [(start + k) % world for k in range(cnt)]
    return rr(0, n_psd), rr(n_psd, n_soc), rr(n_psd + n_soc, n_free)


def variable_owners(prob, owners, soc_owners=None, free_owners=None, world=None):
    """owner rank of every variable: owners[k] for the variables of PSD cone k, soc_owners[j] for SOC cone j,
    free_owners[i] for the i-th free variable (free_variables order).  Lists left out take default_owners' values
    (world defaults to 1 + the largest rank in `owners`)."""
    if soc_owners is None or free_owners is None:
        if world is None:
            world = 1 + max([int(o) for o in owners] + [int(o) for o in (soc_owners or [])] +
                            [int(o) for o in (free_owners or [])] + [0])
        _, dsoc, dfree = default_owners(prob, world)
        soc_owners = dsoc if soc_owners is None else soc_owners
        free_owners = dfree if free_owners is None else free_owners
    free = free_variables(prob)
    if len(owners) != len(prob.psd) or len(soc_owners) != len(prob.soc) or len(free_owners) != len(free):
        raise ValueError("owners / soc_owners / free_owners: one rank per PSD cone / SOC cone / free variable")
    var_owner = np.full(prob.n, -1, dtype=np.int64)
    for lst, own in ((prob.psd, owners), (prob.soc, soc_owners)):
        for k, idx in enumerate(lst):
            idx = np.asarray(idx, dtype=np.int64)
            if np.any(var_owner[idx] >= 0):
                raise ValueError("a variable belongs to more than one cone")
            var_owner[idx] = int(own[k])
    var_owner[free] = np.asarray(free_owners, dtype=np.int64)
    if np.any(var_owner < 0):
        raise ValueError("owner ranks must be >= 0")
    return var_owner


def split_block_diagonal(prob, owners, rank, allow_coupling=True, soc_owners=None, free_owners=None, world=None):
    """Sub-problem of `rank`: the PSD cones with owners[k] == rank (1x1 cones included), the SOC cones with
    soc_owners[j] == rank, the free variables with free_owners[i] == rank (variable_owners; lists left out take the
    deterministic default), the rows of A and G whose entries
    all lie in those variables (PRIVATE rows), and -- SURVEY.md section 8e -- every COUPLING
    row (entries in the variables of more than one shard): each shard carries all coupling rows,
    restricted to its own columns (possibly empty), with the same right-hand side; the partial
    products are summed over the shards once per iteration (proxsdp_problem.coupling_rows).
    A cone is never split.  A row without entries belongs to rank 0.
    Returns (sub-problem, maps); maps["coupling"] = dict(rows, owned) in the shard's row numbering
    (equalities first, then inequalities), or None; maps["psd"] / maps["soc"] the caller's cone numbers the shard
    holds, in the sub-problem's order; maps["vars"] / ["rows_eq"] / ["rows_in"] the caller's variable and row numbers."""
    n = prob.n
    var_owner = variable_owners(prob, owners, soc_owners, free_owners, world)
    mine = np.nonzero(var_owner == rank)[0]
    remap = np.full(n, -1, dtype=np.int64)
    remap[mine] = np.arange(len(mine))

    def rows_of(M):
        M = sp.csr_matrix(M)
        if M.shape[0] == 0:
            z = np.zeros(0, dtype=np.int64)
            return z, sp.csc_matrix((0, len(mine))), z, np.zeros(0, dtype=np.int32)
        row_owner_min = np.full(M.shape[0], np.iinfo(np.int64).max)
        row_owner_max = np.full(M.shape[0], -1)
        coo = M.tocoo()
        np.minimum.at(row_owner_min, coo.row, var_owner[coo.col])
        np.maximum.at(row_owner_max, coo.row, var_owner[coo.col])
        empty = row_owner_max < 0
        row_owner_min[empty] = row_owner_max[empty] = 0
        coupled = row_owner_min != row_owner_max
        if np.any(coupled) and not allow_coupling:
            raise ValueError("a constraint row couples variables of different shards")
        sel = np.nonzero(((row_owner_max == rank) & ~coupled) | coupled)[0]       # original order kept
        local = np.nonzero(coupled[sel])[0]                                      # positions inside `sel`
        owned = (row_owner_min[sel][local] == rank).astype(np.int32)             # the lowest shard of a row owns it
        return sel, sp.csc_matrix(M[sel][:, mine]), local.astype(np.int64), owned

    ra, A, ca, oa = rows_of(prob.A)
    rg, G, cg, og = rows_of(prob.G)
    if soc_owners is None:
        soc_owners = [int(var_owner[np.asarray(idx)[0]]) for idx in prob.soc]
    kpsd = [k for k in range(len(prob.psd)) if int(owners[k]) == rank]
    ksoc = [j for j in range(len(prob.soc)) if int(soc_owners[j]) == rank]
    sub = problems.Problem(n=len(mine), A=A, b=np.asarray(prob.b)[ra], G=G, h=np.asarray(prob.h)[rg],
                           c=np.asarray(prob.c)[mine], psd=[remap[np.asarray(prob.psd[k], dtype=np.int64)] for k in kpsd],
                           soc=[remap[np.asarray(prob.soc[j], dtype=np.int64)] for j in ksoc], max_sense=prob.max_sense,
                           objective_constant=prob.objective_constant, name=f"{prob.name}[shard {rank}]")
    coupling = None
    if len(ca) + len(cg) > 0:
        coupling = dict(rows=np.concatenate([ca, len(ra) + cg]).astype(np.int64),
                        owned=np.concatenate([oa, og]).astype(np.int32))
    return sub, dict(vars=mine, rows_eq=ra, rows_in=rg, coupling=coupling,
                     psd=np.asarray(kpsd, dtype=np.int64), soc=np.asarray(ksoc, dtype=np.int64))


def gather_solution(dist, sol, maps, prob, dst=0):
    """The whole model's result from the shards' (solve_sharded): on rank `dst` a dict with `primal`, `dual_cone` (n),
    `dual_eq`, `slack_eq` (p), `dual_in`, `slack_in` (m) in the caller's variable and row order -- a private row from its
    shard, a coupling row from the shard that owns it -- and None on every other rank.  One gather of the local vectors
    and index maps; every rank must call it."""
    world = dist.get_world_size()
    p_loc = len(maps["rows_eq"])
    own_eq, own_in = np.ones(p_loc, dtype=bool), np.ones(len(maps["rows_in"]), dtype=bool)
    if maps["coupling"] is not None:
        for r, o in zip(maps["coupling"]["rows"], maps["coupling"]["owned"]):
            if r < p_loc:
                own_eq[r] = bool(o)
            else:
                own_in[r - p_loc] = bool(o)
    mine = dict(vars=np.asarray(maps["vars"]), rows_eq=np.asarray(maps["rows_eq"])[own_eq],
                rows_in=np.asarray(maps["rows_in"])[own_in],
                primal=np.asarray(sol.primal), dual_cone=np.asarray(sol.dual_cone),
                dual_eq=np.asarray(sol.dual_eq)[own_eq], slack_eq=np.asarray(sol.slack_eq)[own_eq],
                dual_in=np.asarray(sol.dual_in)[own_in], slack_in=np.asarray(sol.slack_in)[own_in])
    box = [None] * world if dist.get_rank() == dst else None
    dist.gather_object(mine, box, dst=dst)
    if box is None:
        return None
    out = dict(primal=np.zeros(prob.n), dual_cone=np.zeros(prob.n), dual_eq=np.zeros(prob.A.shape[0]),
               slack_eq=np.zeros(prob.A.shape[0]), dual_in=np.zeros(prob.G.shape[0]), slack_in=np.zeros(prob.G.shape[0]))
    seen = {k: np.zeros(len(v), dtype=np.int64) for k, v in out.items() if k in ("primal", "dual_eq", "dual_in")}
    for part in box:
        for key, at in (("primal", "vars"), ("dual_cone", "vars"), ("dual_eq", "rows_eq"), ("slack_eq", "rows_eq"),
                        ("dual_in", "rows_in"), ("slack_in", "rows_in")):
            out[key][part[at]] = part[key]
            if key in seen:
                seen[key][part[at]] += 1
    if any(np.any(v != 1) for v in seen.values()):
        raise ValueError("the shards' maps do not cover every variable and row of the model exactly once")
    return out


class _DevPtr:
    """a raw device pointer as something torch.as_tensor understands (__cuda_array_interface__)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def make_reduce(dist, device=None, world=None):
    """reduce(sums, maxs) over the process group.  ONE collective per call: the packed record
    [sums | maxs] of every rank is all-gathered into a preallocated tensor (on `device` for RCCL, host
    memory for gloo) and combined on the host in rank order -- the same bits on every rank."""
    import torch
    world = world or dist.get_world_size()
    state = {}

    def reduce(sums, maxs):
        ns, nm = len(sums), len(maxs)
        if ns + nm == 0:
            return
        key = (ns, nm)
        if key not in state:
            state[key] = (torch.empty(ns + nm, dtype=torch.float64, device=device or "cpu"),
                          torch.empty(world * (ns + nm), dtype=torch.float64, device=device or "cpu"))
        mine, allr = state[key]
        mine.copy_(torch.from_numpy(np.concatenate([sums, maxs])))
        dist.all_gather_into_tensor(allr, mine)
        rec = allr.cpu().numpy().reshape(world, ns + nm)
        if ns:
            acc = rec[0, :ns].copy()
            for r in range(1, world):
                acc += rec[r, :ns]
            sums[:] = acc
        if nm:
            maxs[:] = rec[:, ns:].max(axis=0)
    return reduce


def make_reduce_vec(dist, device=None):
    """reduce_vec(ptr, length, on_device): element-wise SUM over the process group, in place.  On the
    GPU path `ptr` is a device pointer of the library (a different HIP runtime object than torch's,
    same process, same GPU VM): it is wrapped without a copy and handed to RCCL."""
    import ctypes
    import torch

    def reduce_vec(ptr, length, on_device):
        if on_device:
            t = torch.as_tensor(_DevPtr(ptr, length), device=device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize(device)
        else:
            buf = (ctypes.c_double * length).from_address(ptr)
            t = torch.from_numpy(np.ctypeslib.as_array(buf))
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return reduce_vec


def make_native_comm(dist, rank, world, device_id=0):
    """RCCL communicator for the library's NATIVE collectives (proxsdp_problem.nccl_comm): rank 0 draws the
    unique id through the library's own librccl, the 128 bytes travel over the existing process group (any
    backend), every rank joins on the GPU it owns.  torch.distributed's communicator is not reachable from
    outside torch, and a communicator must belong to the librccl that issues the calls."""
    from . import binding
    box = [binding.rccl_unique_id() if rank == 0 else None]
    if world > 1:
        dist.broadcast_object_list(box, src=0)
    return binding.rccl_comm_init(world, box[0], rank, device_id)


def solve_sharded(prob, dist, rank, world, device_id=0, owners=None, collective_device=None, native_comm=None,
                  soc_owners=None, free_owners=None, **options):
    """Every rank calls this with the SAME full model; returns (Optimizer, SolveResult of the
    local shard, index maps).  Objective / gap / status are global and identical on all ranks; gather_solution
    reassembles the vectors.  owners / soc_owners / free_owners: rank per PSD cone / SOC cone / free variable
    (default_owners when left out); every cone class the single-process solve accepts is accepted.
    native_comm: handle from make_native_comm -> the library reduces scalars and coupling rows itself over RCCL
    on its own stream (no Python callback per iteration); otherwise the torch.distributed callbacks below
    (the path the gloo tests use).
    A failure on one rank (bad model, a rank that would own nothing, an error inside the library) is
    all-reduced before anybody enters the solve loop's collectives, so all ranks raise together
    instead of leaving the others blocked in an all-reduce."""
    import torch
    err = None
    sub = maps = None
    try:
        d_psd, d_soc, d_free = default_owners(prob, world)
        owners = owners if owners is not None else d_psd
        soc_owners = soc_owners if soc_owners is not None else d_soc
        free_owners = free_owners if free_owners is not None else d_free
        held = np.bincount(variable_owners(prob, owners, soc_owners, free_owners), minlength=world)
        if len(held) > world or np.any(held[:world] == 0):
            raise ValueError(f"{world} ranks, variables per rank {held.tolist()}: every rank must own at least one "
                             "variable, and no owner may lie outside the ranks")
        sub, maps = split_block_diagonal(prob, owners, rank, soc_owners=soc_owners, free_owners=free_owners)
    except Exception as e:                                   # noqa: BLE001 -- re-raised below on every rank
        err = e
    flag = torch.tensor([1.0 if err is not None else 0.0], dtype=torch.float64,
                        device=collective_device or "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if float(flag.item()) > 0:
        raise err if err is not None else RuntimeError("another rank failed to build its shard")
    opt = Optimizer(device_id=device_id, **options)
    coupling = None
    tcap = int(options.get("max_iter", 0)) if options.get("max_iter", 0) else 0
    if native_comm:
        if maps["coupling"] is not None:
            coupling = dict(maps["coupling"])
        sol = opt.optimize(sub, coupling=coupling, nccl_comm=native_comm, trace_capacity=tcap)
        return opt, sol, maps
    if maps["coupling"] is not None:
        coupling = dict(maps["coupling"], reduce_vec=make_reduce_vec(dist, collective_device),
                        on_device=collective_device is not None)
    sol = opt.optimize(sub, reduce=make_reduce(dist, collective_device, world), coupling=coupling, trace_capacity=tcap)
    return opt, sol, maps
