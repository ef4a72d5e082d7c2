"""Block-sharded solve of mixed-cone models: SOC cones, 1x1 PSD blocks and free variables beside PSD blocks (a shard
with any of them, or without a PSD block, runs the library's general vector path; stats["sharded_general_iterations"] says
so).  Ranks are spawned as in test_sharded_gpu.py: gloo, all ranks on the one GPU of the test box, at most three.

The contract against the single-process solve is that file's (test_two_shards_reproduce_the_single_process_solve): same
status and iteration count, the same linesearch trials in every iteration, trace columns 1, 2, 7 (objectives, primal step)
to rtol 1e-9 / atol 1e-12, the reassembled primal to 1e-9, objectives to 1e-9 relative."""
import math
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import GOLDEN
from kat_problems import mixed_cones, sdp_plus_soc
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd.optimizer import Optimizer

import vector_kernel_cases as V

pytestmark = pytest.mark.gpu


def _couple(pr, d00, d11):
    """one equality and one inequality that touch the first block and a block behind it, as test_sharded_gpu._coupled_model
    builds them: X1[0,0] + 2 X2[0,0] = 3 and X1[1,1] - X2[1,1] <= 0.5 (variables 0 and 2 are entries (0,0) and (1,1) of the
    first block's triangle, d00 and d11 those of the other block)"""
    import scipy.sparse as sp
    row = sp.csr_matrix(([1.0, 2.0], ([0, 0], [0, d00])), shape=(1, pr.n))
    g = sp.csr_matrix(([1.0, -1.0], ([0, 0], [2, d11])), shape=(1, pr.n))
    return P.Problem(n=pr.n, A=sp.vstack([pr.A, row]).tocsc(), b=np.append(pr.b, 3.0),
                     G=sp.vstack([pr.G, g]).tocsc(), h=np.append(pr.h, 0.5), c=pr.c, psd=pr.psd, soc=pr.soc,
                     name=pr.name + "-coupled")


def _model(key):
    """(model, owners, soc_owners, free_owners); None = the deterministic default"""
    kind, _, arg = key.partition(":")
    if kind == "mixed":                                   # sides (1, 3, 104, 1, 5), one SOC, three free variables
        return mixed_cones(int(arg)), None, None, None
    if kind == "mixed3":                                  # three ranks, rank 2 holds only the SOC and the free variables
        pr = mixed_cones(int(arg))
        return pr, [0, 1, 0, 1, 1], [2], [2, 2, 2]
    if kind == "sdplib":
        return P.sdplib_blocks(GOLDEN / "sdplib" / f"{arg}.dat-s"), None, None, None
    if kind == "paths":                                   # rank 0: the Max-Cut block alone (support path); rank 1: the rest
        mc, mx = P.maxcut(120, seed=1), mixed_cones(2)
        big = mx.psd[2]                                   # the 104 x 104 block of the mixed model (its variable ids are shuffled)
        pr = _couple(P.block_diag_problems([mc, mx], name="maxcut-mixed"), mc.n + big[0], mc.n + big[2])
        return pr, [0] + [1] * len(mx.psd), [1], [1] * 3
    if kind == "socstop":                                 # rank 0: sdp_plus_soc (PSD + SOC + free); rank 1: a small Max-Cut
        pr = P.block_diag_problems([sdp_plus_soc(), P.maxcut(20, seed=3)], name="soc-maxcut")
        return pr, [0, 1], [0], [0]
    raise KeyError(key)


def _worker(rank, world, port, q, key, options, gather, fail_rank):
    env = dict(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if fail_rank is not None:
        env["PROXSDP_HIP_FAULT_INJECTION"] = "1"
    os.environ.update(env)
    from proxsdp_jl_amd import replicas, sharded
    dist = replicas.init("gloo", rank, world)
    pr, owners, soc_owners, free_owners = _model(key)
    kw = dict(options)
    if fail_rank == rank:
        kw["debug_fail_iteration"] = 7                    # this shard's projection throws in iteration 7
    try:
        opt, sol, maps = sharded.solve_sharded(pr, dist, rank, world, device_id=0, owners=owners, soc_owners=soc_owners,
                                               free_owners=free_owners, **kw)
    except B.ProxSDPHipError as e:
        q.put((rank, str(e)))
        dist.destroy_process_group()
        return
    whole = sharded.gather_solution(dist, sol, maps, pr, dst=0) if gather else None
    q.put((rank, dict(status=sol.status, iter=int(sol.iter), objval=sol.objval, dual_objval=sol.dual_objval,
                      final_rank=int(sol.final_rank), vars=maps["vars"], primal=sol.primal,
                      trace=sol.trace[:, [1, 2, 7, 11, 12]], stats=sol.stats, whole=whole,
                      n_psd=len(maps["psd"]), n_soc=len(maps["soc"]), psd=maps["psd"])))
    dist.destroy_process_group()


_PORT_SLOT = iter(range(1000))


def _spawn(key, world, options, gather=False, fail_rank=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 20000 + (os.getpid() % 2000) + 2000 * (1 + next(_PORT_SLOT) % 12)
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, key, options, gather, fail_rank)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)         # a hang shows up as queue.Empty here
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [out[r] for r in range(world)]


def _contract(pr, ref, out):
    x = np.full(pr.n, np.nan)
    for o in out:
        assert o["status"] == ref.status and o["iter"] == ref.iter, (o["status"], ref.status, o["iter"], ref.iter)
        assert np.array_equal(o["trace"][:, 3], ref.trace[:, 11])                       # same linesearch trials
        R = ref.trace[:, [1, 2, 7]]
        excess = np.abs(o["trace"][:, :3] - R) / (1e-12 + 1e-9 * np.abs(R))
        print("trace columns 1, 2, 7: largest |difference| / (atol + rtol |ref|) = %.3g at iteration %d; first iteration above 1: %s"
              % (excess.max(), 1 + int(np.argmax(excess.max(axis=1))), (1 + np.nonzero(excess.max(axis=1) > 1)[0][:1]).tolist()))
        assert np.allclose(o["trace"][:, :3], ref.trace[:, [1, 2, 7]], rtol=1e-9, atol=1e-12)
        assert abs(o["objval"] - ref.objval) <= 1e-9 * (1 + abs(ref.objval))
        assert abs(o["dual_objval"] - ref.dual_objval) <= 1e-9 * (1 + abs(ref.dual_objval))
        x[o["vars"]] = o["primal"]
    assert np.allclose(x, ref.primal, rtol=0, atol=1e-9)


def _general_path(o):
    return o["stats"]["sharded_general_iterations"] == o["iter"]


# ----------------------------------------------------------------- Test 1
def test_one_shard_is_the_plain_solve_bit_for_bit():
    """one shard, no coupling rows, the identity as reduce: every kernel sees the plain solve's inputs"""
    assert B.device_count() > 0
    pr = mixed_cones(0)
    ref = Optimizer(max_iter=300).optimize(pr, trace_capacity=300)
    sol = Optimizer(max_iter=300).optimize(pr, trace_capacity=300, reduce=lambda sums, maxs: None)
    assert sol.iter == ref.iter and sol.status == ref.status
    assert np.array_equal(sol.primal, ref.primal)
    cols = [c for c in range(ref.trace.shape[1]) if c != 12]            # 12: elapsed seconds
    assert sol.trace.shape == ref.trace.shape and np.array_equal(sol.trace[:, cols], ref.trace[:, cols])
    assert sol.stats["sharded_general_iterations"] == sol.iter and ref.stats["sharded_general_iterations"] == 0
    small = lambda s: (s.stats["batched_small_eigs"], s.stats["full_eigs_sign"], s.stats["sign_short_pass"], s.stats["sign_short_fail"])
    assert sol.stats["batched_small_eigs"] > 0 and small(sol) == small(ref)           # the one-launch small-block projections


# ----------------------------------------------------------------- Tests 2, 4, 6
@pytest.mark.parametrize("key,world", [("mixed:0", 2), ("mixed:1", 2), ("mixed3:0", 3), ("sdplib:truss1", 2), ("sdplib:control1", 2)])
def test_shards_reproduce_the_single_process_solve(key, world):
    assert B.device_count() > 0
    pr = _model(key)[0]
    ref = Optimizer(max_iter=300).optimize(pr, trace_capacity=300)
    out = _spawn(key, world, dict(max_iter=300))
    _contract(pr, ref, out)
    sides = np.asarray(pr.psd_sides())
    for o in out:
        # a shard with an SOC, a 1x1 block or no PSD block ran the general path; any other one the support path, as before
        # (control1: two blocks of side 10 and 5, one per rank -- the one model of this list that sharded before)
        print(key, "psd sides", sides[o["psd"]].tolist(), "soc", o["n_soc"], "general iterations", o["stats"]["sharded_general_iterations"])
        general = o["n_soc"] > 0 or o["n_psd"] == 0 or bool(np.any(sides[o["psd"]] == 1))
        assert o["stats"]["sharded_general_iterations"] == (o["iter"] if general else 0)
    assert any(_general_path(o) for o in out) or key == "sdplib:control1"
    if key.startswith("mixed3"):
        assert out[2]["n_psd"] == 0 and out[2]["n_soc"] == 1 and _general_path(out[2])


# ----------------------------------------------------------------- Test 3
def test_support_path_and_general_path_shards_in_one_solve():
    assert B.device_count() > 0
    pr = _model("paths")[0]
    ref = Optimizer(max_iter=300).optimize(pr, trace_capacity=300)
    out = _spawn("paths", 2, dict(max_iter=300))
    _contract(pr, ref, out)
    assert out[0]["stats"]["sharded_general_iterations"] == 0 and out[0]["stats"]["fop_projections"] + out[0]["stats"]["lanczos_matvecs"] > 0
    assert out[1]["stats"]["sharded_general_iterations"] == out[1]["iter"]


# ----------------------------------------------------------------- Test 5
def test_to_the_optimum_through_the_gather_helper():
    assert B.device_count() > 0
    pr = mixed_cones(0)
    ref = Optimizer().optimize(pr, trace_capacity=2000)
    assert ref.status == 1
    out = _spawn("mixed:0", 2, dict(trace_capacity=2000), gather=True)
    assert out[1]["whole"] is None
    g = out[0]["whole"]
    sc = max(1.0, np.abs(ref.primal).max())
    for o in out:
        print("rank iterations", o["iter"], "single process", ref.iter, "per iteration: %.1f us sharded, %.1f us single"
              % (1e6 * o["trace"][-1, 4] / o["iter"], 1e6 * ref.trace[-1, 12] / ref.iter))
        assert o["status"] == 1
        assert abs(o["iter"] - ref.iter) <= max(3, 0.05 * ref.iter)
        assert abs(o["objval"] - ref.objval) <= 2e-6 * (1 + abs(ref.objval))
        assert o["final_rank"] == ref.final_rank
    for k in ("primal", "slack_eq", "slack_in", "dual_eq", "dual_in"):
        assert np.allclose(g[k], getattr(ref, k), rtol=0, atol=2e-5 * sc), k
    for idx, side in zip(pr.psd, pr.psd_sides()):
        assert np.linalg.eigvalsh(P.unpack_psd(g["primal"][idx], side)).min() >= -1e-6
    t = g["primal"][pr.soc[0]]
    assert t[0] >= np.linalg.norm(t[1:]) - 1e-6


# ----------------------------------------------------------------- Test 7
def test_soc_stop_rule_is_global():
    """sdp_plus_soc on rank 0, a small Max-Cut on rank 1, solved to tolerance: the SOC-free rank must neither stop before
    the SOC gap of the other rank is closed nor wait for ever in a collective the other rank never enters"""
    assert B.device_count() > 0
    pr = _model("socstop")[0]
    ref = Optimizer().optimize(pr)
    assert ref.status == 1
    out = _spawn("socstop", 2, dict())
    for o in out:
        assert o["status"] == 1 and o["iter"] == ref.iter, (o["iter"], ref.iter)
        assert abs(o["objval"] - ref.objval) <= 1e-9 * (1 + abs(ref.objval))
    assert out[0]["n_soc"] == 1 and out[1]["n_soc"] == 0


# ----------------------------------------------------------------- Test 8
def test_a_failing_general_path_shard_makes_every_shard_abort():
    out = _spawn("mixed:0", 2, dict(max_iter=300), fail_rank=1)
    assert isinstance(out[0], str) and isinstance(out[1], str), out
    assert "injected projection failure" in out[1], out
    assert "another shard" in out[0], out


# ----------------------------------------------------------------- Test 9: the weighted general residual, kernel level
def _weighted_case(Q, p, zero_rows, seed):
    rng = np.random.default_rng(seed)
    n = 130
    lens = np.minimum(V.short_lengths(n, rng), Q)
    cs = V.make_case(f"weighted_Q{Q}_p{p}", Q, lens, p, seed)
    w = np.ones(Q)
    w[np.asarray(zero_rows, dtype=np.int64)] = 0.0
    cs["roww"] = w
    return cs


WEIGHTED = {
    "Q1": (1, 0, [0]),
    "Q1-eq": (1, 1, [0]),
    "Q255": (255, 100, [0, 254]),
    "Q256": (256, 131, [0, 255]),
    "Q257": (257, 256, [0, 255, 256]),                      # the only inequality row sits alone in the second workgroup
    "Q700": (700, 300, [0, 255, 256, 511, 512, 699]),       # first and last row of each of the three workgroups
    "Q700-ineq-off": (700, 300, list(range(300, 700))),     # every inequality row on another shard
}


def _check(got, maxs, sums, what):
    for q in range(V.NSCAL):
        if q in maxs:
            assert got[q] == maxs[q], (what, q, got[q], maxs[q])
        else:
            exact, bound = math.fsum(sums[q]), V.sum_bound(sums[q])
            print(f"{what} slot {q}: |got - fsum| = {abs(got[q] - exact):.3e}, bound {bound:.3e}")
            assert abs(got[q] - exact) <= bound, (what, q, got[q], exact, bound)


@pytest.mark.parametrize("plain", [False, True], ids=["linesearch", "plain"])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("name", list(WEIGHTED))
def test_weighted_general_residual_kernel_level(name, nc, plain):
    """proxsdp_hip_trial_batch, general path, with the switch a block-sharded solve sets (support = 2): b'y and h'y count
    the rows with weight 1 only; y+, M'y+ and the maxima as without it.  Without the switch the same inputs give the
    unweighted sums, as before."""
    assert B.device_count() > 0
    Q, p, zero_rows = WEIGHTED[name]
    cs = _weighted_case(Q, p, zero_rows, 500 + Q + p)
    ref = V.reference(cs, nc=nc, plain=plain, support=False)
    args = V.hook_args(cs, nc=nc, plain=plain, support=False)
    w = cs["roww"]
    for switch in (True, False):
        out = B.trial_batch(cs["colptr"], cs["row"], cs["val"], cs["Q"], sharded_rows=switch, **args)
        for k in range(nc):
            assert np.array_equal(out["y"][k].view(np.uint64), ref["y"][k].view(np.uint64))
            assert np.array_equal(out["Mty"][k].view(np.uint64), ref["Mty"][k].view(np.uint64))
            sums = dict(ref["sums"][k])
            if switch:                                     # (1.0 * t == t: the unweighted terms times the weights are the kernel's)
                sums[9], sums[10] = w[:p] * sums[9], w[p:] * sums[10]
            _check(out["scal"][k], ref["maxs"][k], sums, f"{name} nc={nc} plain={plain} switch={switch} candidate {k}")
    if name == "Q700-ineq-off":
        out = B.trial_batch(cs["colptr"], cs["row"], cs["val"], cs["Q"], sharded_rows=True, **args)
        assert np.all(out["scal"][:, 10] == 0.0)
