"""Host side of the block-sharded solve (proxsdp_jl_amd/sharded.py), no GPU: splitting a model with every cone class --
PSD blocks of any side (1x1 included), SOC cones, free variables -- over the ranks, and putting the shards' results back
together (gather_solution)."""
import multiprocessing as mp
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN
from kat_problems import mixed_cones, sdp_plus_soc
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd import sharded


def _model(name):
    if name == "truss1":
        return P.sdplib_blocks(GOLDEN / "sdplib" / "truss1.dat-s")
    return mixed_cones(int(name))


def _explicit_owners(pr, world):
    """an assignment unlike the default one: cones dealt out from the last rank down, every free variable on the last rank"""
    own = lambda cnt, shift: [(world - 1 - (k + shift)) % world for k in range(cnt)]
    return own(len(pr.psd), 0), own(len(pr.soc), 1), [world - 1] * len(sharded.free_variables(pr))


@pytest.mark.parametrize("explicit", [False, True], ids=["default-owners", "explicit-owners"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["0", "1", "2", "3", "truss1"])
def test_split_covers_the_model_exactly_once(name, world, explicit):
    pr = _model(name)
    if explicit:
        owners, soc_owners, free_owners = _explicit_owners(pr, world)
    else:
        owners, soc_owners, free_owners = sharded.default_owners(pr, world)
        assert (owners, soc_owners, free_owners) == sharded.default_owners(pr, world)      # the same map on every rank
    kw = dict(soc_owners=soc_owners, free_owners=free_owners) if explicit else dict(world=world)
    shards = [sharded.split_block_diagonal(pr, owners, r, **kw) for r in range(world)]
    M = sp.vstack([pr.A, pr.G]).tocsr()
    p, Q = pr.A.shape[0], M.shape[0]
    rhs = np.concatenate([pr.b, pr.h])

    # every variable is owned exactly once
    var_count = np.zeros(pr.n, dtype=int)
    for sub, maps in shards:
        var_count[maps["vars"]] += 1
        assert sub.n == len(maps["vars"])
    assert np.all(var_count == 1)

    # no cone is split: every cone is whole on exactly one shard, in the caller's entry order
    for attr in ("psd", "soc"):
        held = np.zeros(len(getattr(pr, attr)), dtype=int)
        for sub, maps in shards:
            assert len(getattr(sub, attr)) == len(maps[attr])
            for loc, k in zip(getattr(sub, attr), maps[attr]):
                held[k] += 1
                assert np.array_equal(maps["vars"][loc], getattr(pr, attr)[k])
        assert np.all(held == 1)

    # every row is private to one shard or a coupling row carried by all; each coupling row is owned exactly once
    carried = np.zeros(Q, dtype=int)
    is_coupling = np.zeros(Q, dtype=int)
    owned = np.zeros(Q, dtype=int)
    for sub, maps in shards:
        rows = np.concatenate([maps["rows_eq"], p + maps["rows_in"]])
        carried[rows] += 1
        if maps["coupling"] is not None:
            cr = rows[maps["coupling"]["rows"]]
            is_coupling[cr] += 1
            owned[cr] += maps["coupling"]["owned"]
    assert np.all((carried == 1) | (carried == world))
    assert np.all(is_coupling[carried == world] == world) or world == 1
    assert np.all(is_coupling[carried == 1] == 0)
    assert np.all(owned[is_coupling > 0] == 1) and np.all(owned[is_coupling == 0] == 0)
    # (every shard lists the coupling rows in the same order: the caller's)
    lists = [np.concatenate([m["rows_eq"], p + m["rows_in"]])[m["coupling"]["rows"]] for _, m in shards if m["coupling"] is not None]
    assert all(np.array_equal(lists[0], L) for L in lists)
    # a coupling row has entries in more than one shard, a private row in one
    var_owner = sharded.variable_owners(pr, owners, soc_owners, free_owners)
    for r in range(Q):
        ranks = set(var_owner[M.indices[M.indptr[r]:M.indptr[r + 1]]].tolist())
        assert (len(ranks) > 1) == bool(is_coupling[r]), r

    # stacking the shards' columns reproduces [A;G], b, h, c entry for entry
    full = sp.lil_matrix((Q, pr.n))
    c = np.full(pr.n, np.nan)
    got_rhs = np.full(Q, np.nan)
    for sub, maps in shards:
        rows = np.concatenate([maps["rows_eq"], p + maps["rows_in"]])
        blk = sp.vstack([sub.A, sub.G]).tocoo()
        full[rows[blk.row], maps["vars"][blk.col]] = blk.data
        c[maps["vars"]] = sub.c
        sub_rhs = np.concatenate([sub.b, sub.h])
        assert np.all(np.isnan(got_rhs[rows]) | (got_rhs[rows] == sub_rhs))         # a coupling row: the same rhs everywhere
        got_rhs[rows] = sub_rhs
        assert sub.A.shape == (len(maps["rows_eq"]), sub.n) and sub.G.shape == (len(maps["rows_in"]), sub.n)
    assert (full.tocsr() != M).nnz == 0
    assert sum(sp.vstack([s.A, s.G]).nnz for s, _ in shards) == M.nnz
    assert np.array_equal(c, pr.c) and np.array_equal(got_rhs, rhs)


def test_models_that_sharded_before_split_as_before():
    """PSD blocks of side >= 2 only: owners alone decide, no SOC / free list is needed, maps keep their keys"""
    pr = P.block_diag_problems([P.maxcut(12, seed=1), P.maxcut(15, seed=2)])
    for r in range(2):
        sub, maps = sharded.split_block_diagonal(pr, [0, 1], r)
        assert maps["coupling"] is None and len(sub.psd) == 1 and not sub.soc
        assert np.array_equal(maps["vars"], pr.psd[r]) and np.array_equal(maps["psd"], [r]) and len(maps["soc"]) == 0
    with pytest.raises(ValueError, match="couples"):
        row = sp.csr_matrix(([1.0, 1.0], ([0, 0], [0, pr.n - 1])), shape=(1, pr.n))
        bad = P.Problem(n=pr.n, A=sp.vstack([pr.A, row]).tocsc(), b=np.append(pr.b, 1.0), G=pr.G, h=pr.h, c=pr.c, psd=pr.psd)
        sharded.split_block_diagonal(bad, [0, 1], 0, allow_coupling=False)


class _Sol:
    pass


def _gather_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from proxsdp_jl_amd import replicas
    dist = replicas.init("gloo", rank, world)
    pr = mixed_cones(1, sides=(1, 3, 6, 1, 5), p=10, m=6)
    owners, soc_owners, free_owners = sharded.default_owners(pr, world)
    sub, maps = sharded.split_block_diagonal(pr, owners, rank, world=world)
    # synthetic shard results: entry = a function of the caller's variable / row number; on a coupling row the dual and the
    # slack are the same on every shard (as the library leaves them), marked so that only the OWNER's copy is right
    sol = _Sol()
    sol.primal, sol.dual_cone = 1.0 + maps["vars"], -1.0 - maps["vars"]
    sol.dual_eq, sol.slack_eq = 100.0 + maps["rows_eq"], 200.0 + maps["rows_eq"]
    sol.dual_in, sol.slack_in = 300.0 + maps["rows_in"], 400.0 + maps["rows_in"]
    p_loc = len(maps["rows_eq"])
    assert maps["coupling"] is not None
    for r, o in zip(maps["coupling"]["rows"], maps["coupling"]["owned"]):
        if not o:
            for a in ((sol.dual_eq, sol.slack_eq) if r < p_loc else (sol.dual_in, sol.slack_in)):
                a[r if r < p_loc else r - p_loc] = np.nan
    out = sharded.gather_solution(dist, sol, maps, pr, dst=0)
    q.put((rank, out))
    dist.destroy_process_group()


def test_gather_solution_returns_the_whole_model_on_the_destination_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29100 + (os.getpid() % 300)
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out[1] is None
    pr = mixed_cones(1, sides=(1, 3, 6, 1, 5), p=10, m=6)
    g = out[0]
    assert sorted(g) == ["dual_cone", "dual_eq", "dual_in", "primal", "slack_eq", "slack_in"]
    assert np.array_equal(g["primal"], 1.0 + np.arange(pr.n)) and np.array_equal(g["dual_cone"], -1.0 - np.arange(pr.n))
    assert np.array_equal(g["dual_eq"], 100.0 + np.arange(pr.p)) and np.array_equal(g["slack_eq"], 200.0 + np.arange(pr.p))
    assert np.array_equal(g["dual_in"], 300.0 + np.arange(pr.m)) and np.array_equal(g["slack_in"], 400.0 + np.arange(pr.m))


def _empty_rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from proxsdp_jl_amd import replicas
    dist = replicas.init("gloo", rank, world)
    pr = sdp_plus_soc()                                       # one PSD block, one SOC, one free variable
    try:
        # every cone and the free variable on rank 0: rank 1 would own nothing.  Nobody reaches the library.
        sharded.solve_sharded(pr, dist, rank, world, owners=[0], soc_owners=[0], free_owners=[0], max_iter=5)
        q.put((rank, "returned"))
    except ValueError as e:
        q.put((rank, str(e)))
    dist.destroy_process_group()


def test_a_rank_that_would_own_nothing_makes_all_ranks_raise_together():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29100 + (os.getpid() % 300) + 311
    procs = [ctx.Process(target=_empty_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all("every rank must own at least one variable" in out[r] for r in range(2)), out
