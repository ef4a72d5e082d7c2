"""Host side of the block-sharded solve from one call (proxsdp_hip_solve_sharded), no GPU: the library's own split of a
model into shards (csrc/shard_split.hpp) against sharded.split_block_diagonal, and the in-process group's scalar reduce
(csrc/shard_group.hpp: barrier + combine in shard order) with its abandon path."""
import math
import multiprocessing as mp

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN
from kat_problems import mixed_cones, sdp_plus_soc
from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P
from proxsdp_jl_amd import sharded


def _model(name):
    if name == "truss1":
        return P.sdplib_blocks(GOLDEN / "sdplib" / "truss1.dat-s")
    return mixed_cones(int(name))


def _explicit_owners(pr, world):
    """tests/test_sharded_split_host.py's assignment: cones dealt out from the last rank down, free variables on the last"""
    own = lambda cnt, shift: [(world - 1 - (k + shift)) % world for k in range(cnt)]
    return own(len(pr.psd), 0), own(len(pr.soc), 1), [world - 1] * len(sharded.free_variables(pr))


def _canon(M):
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sort_indices()
    return M


def _same_csc(got, ref):
    ref = _canon(ref)
    assert got.shape == ref.shape
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert np.array_equal(got.data, ref.data)


# ----------------------------------------------------------------- the C++ split against the Python split
@pytest.mark.parametrize("index_base", [0, 1])
@pytest.mark.parametrize("explicit", [False, True], ids=["default-owners", "explicit-owners"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["0", "1", "2", "3", "truss1"])
def test_library_split_equals_the_python_split(name, world, explicit, index_base):
    pr = _model(name)
    owners = soc_owners = free_owners = None
    if explicit:
        owners, soc_owners, free_owners = _explicit_owners(pr, world)
    py_owners = owners if explicit else sharded.default_owners(pr, world)[0]
    kw = dict(soc_owners=soc_owners, free_owners=free_owners) if explicit else dict(world=world)
    n_coupling = 0
    for r in range(world):
        sub, maps = sharded.split_block_diagonal(pr, py_owners, r, **kw)
        got = B.host_split_shard(pr, world, r, owners=owners, soc_owners=soc_owners, free_owners=free_owners,
                                 index_base=index_base)
        for key in ("vars", "rows_eq", "rows_in"):
            assert np.array_equal(got[key], maps[key]), key
        cp = maps["coupling"] or dict(rows=np.zeros(0, dtype=np.int64), owned=np.zeros(0, dtype=np.int32))
        assert np.array_equal(got["coupling_rows"], cp["rows"]) and np.array_equal(got["coupling_owned"], cp["owned"])
        n_coupling += len(cp["rows"])
        _same_csc(got["A"], sub.A)
        _same_csc(got["G"], sub.G)
        assert np.array_equal(got["b"], sub.b) and np.array_equal(got["h"], sub.h) and np.array_equal(got["c"], sub.c)
        assert np.array_equal(got["psd_ids"], maps["psd"]) and np.array_equal(got["soc_ids"], maps["soc"])
        for kind in ("psd", "soc"):
            assert len(got[kind]) == len(getattr(sub, kind))
            for a, b in zip(got[kind], getattr(sub, kind)):
                assert np.array_equal(a, b)
    if name != "truss1":
        assert n_coupling > 0                                # the mixed models have rows across shards: that branch ran


@pytest.mark.parametrize("index_base", [0, 1])
def test_start_vectors_are_split_per_cone(index_base):
    """eig_resid holds one start vector per PSD cone, sides concatenated in the caller's cone order: a shard gets the vectors
    of its own cones, in that order -- here with the cones of every shard interleaved in the caller's order"""
    pr = mixed_cones(0)
    sides = pr.psd_sides()
    er = [100.0 * k + np.arange(1, side + 1) for k, side in enumerate(sides)]           # every entry names its cone and position
    for world, owners in ((2, [1, 0, 1, 0, 0]), (3, [2, 0, 1, 0, 2])):
        soc_owners, free_owners = [1] * len(pr.soc), [1] * len(sharded.free_variables(pr))
        seen = 0
        for r in range(world):
            got = B.host_split_shard(pr, world, r, owners=owners, soc_owners=soc_owners, free_owners=free_owners,
                                     index_base=index_base, eig_resid=er)
            mine = [k for k, o in enumerate(owners) if o == r]
            assert np.array_equal(got["psd_ids"], mine)
            assert np.array_equal(got["eig_resid"], np.concatenate([er[k] for k in mine]))
            seen += len(got["eig_resid"])
            assert len(B.host_split_shard(pr, world, r, owners=owners, soc_owners=soc_owners, free_owners=free_owners,
                                          index_base=index_base)["eig_resid"]) == 0     # none given, none out
        assert seen == sum(sides)


def test_a_row_without_entries_belongs_to_shard_0():
    pr = P.block_diag_problems([P.maxcut(5, seed=1), P.maxcut(6, seed=2)])
    A = sp.vstack([pr.A, sp.csr_matrix((1, pr.n))]).tocsc()
    G = sp.csr_matrix(([1.0, 1.0], ([1, 1], [0, pr.n - 1])), shape=(2, pr.n)).tocsc()      # row 0 empty, row 1 couples
    pr2 = P.Problem(n=pr.n, A=A, b=np.append(pr.b, 0.0), G=G, h=np.array([0.0, 1.0]), c=pr.c, psd=pr.psd)
    for r in range(2):
        sub, maps = sharded.split_block_diagonal(pr2, [0, 1], r)
        got = B.host_split_shard(pr2, 2, r, owners=[0, 1])
        assert np.array_equal(got["rows_eq"], maps["rows_eq"]) and np.array_equal(got["rows_in"], maps["rows_in"])
        assert (pr2.A.shape[0] - 1 in got["rows_eq"]) == (r == 0) and (0 in got["rows_in"]) == (r == 0)
        assert np.array_equal(got["coupling_rows"], maps["coupling"]["rows"])
        assert np.array_equal(got["coupling_owned"], maps["coupling"]["owned"]) and got["coupling_owned"][0] == (r == 0)


def _rejected(match, *args, **kw):
    with pytest.raises(B.ProxSDPHipError, match=match) as e:
        B.host_split_shard(*args, **kw)
    assert e.value.code == -1                               # PROXSDP_E_INVALID


def test_rejected_inputs():
    pr = sdp_plus_soc()                                      # one PSD block, one SOC, one free variable
    _rejected("would own no variable", pr, 2, 0, owners=[0], soc_owners=[0], free_owners=[0])
    _rejected("would own no variable", pr, 4, 0)             # three things to own, four shards
    _rejected("owner outside", pr, 2, 0, owners=[2], soc_owners=[0], free_owners=[1])
    _rejected("owner outside", pr, 2, 0, owners=[0], soc_owners=[-1], free_owners=[1])
    _rejected("shard outside", pr, 2, 2)
    _rejected("n_shards", pr, 0, 0)
    # a variable in two cones: the SOC takes a variable of the PSD block
    soc = [np.concatenate([[pr.psd[0][0]], np.asarray(pr.soc[0])[1:]])]
    bad = P.Problem(n=pr.n, A=pr.A, b=pr.b, G=pr.G, h=pr.h, c=pr.c, psd=pr.psd, soc=soc)
    _rejected("more than one cone", bad, 2, 0)
    # the model must be whole: a reduce callback marks it as a shard of some other solve
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)

    def as_shard(Pm):
        Pm.reduce_fn = B.C.cast(cb, B.C.c_void_p)
    _rejected("must not itself be a shard", pr, 2, 0, raw_problem=as_shard)

    def with_coupling(Pm):
        Pm.n_coupling = 1
    _rejected("must not itself be a shard", pr, 2, 0, raw_problem=with_coupling)

    def with_dense_a(Pm):                                    # (never read: a non-NULL pointer is all the check looks at)
        Pm.M_dense = B.C.c_void_p(8)
    _rejected("A_dense cannot be combined", pr, 2, 0, raw_problem=with_dense_a)


# ----------------------------------------------------------------- the in-process reduce alone
def _records(S, K, nsum, nmax, seed):
    """values where the order of addition shows: 1e16, 1, -1e16 dealt over the shards, small integers elsewhere"""
    rng = np.random.default_rng(seed)
    rec = rng.integers(-3, 4, size=(K, S, nsum + nmax)).astype(np.float64)
    big = np.array([1e16, 1.0, -1e16, 3.0, 1.0, 1.0, -1.0, 1e16])
    for k in range(K):
        rec[k, :, 0] = np.roll(big, k)[:S]
        rec[k, :, 1] = np.roll(big[::-1], k)[:S]
    rec[:, :, nsum] = rng.standard_normal((K, S))
    rec[0, 0, nsum + 1] = -0.0
    return rec


def _shard_order(rec, nsum):
    K, S, w = rec.shape
    out = np.zeros((K, w))
    for k in range(K):
        acc = rec[k, 0, :nsum].copy()
        for r in range(1, S):
            acc += rec[k, r, :nsum]
        out[k, :nsum] = acc
        out[k, nsum:] = rec[k, :, nsum:].max(axis=0)
    return out


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_group_reduce_combines_in_shard_order(S):
    K, nsum, nmax = 40, 5, 3
    rec = _records(S, K, nsum, nmax, seed=S)
    exp = _shard_order(rec, nsum)
    if S == 3:                                               # the order shows: (1e16 + 1) - 1e16 = 0, the exact sum is 1
        assert exp[0, 0] == 0.0 and math.fsum(rec[0, :, 0]) == 1.0
    out, done, failed = B.host_group_reduce(rec, nsum)
    assert np.all(done == K) and not np.any(failed)
    for s in range(S):                                       # every shard holds the same bits
        assert np.array_equal(out[s, :, :nsum], exp[:, :nsum]), s
        assert np.array_equal(out[s, :, nsum:], exp[:, nsum:]), s


def _abandon_child(q, S, leave_shard, leave_after):
    rec = _records(S, 12, 4, 2, seed=11)
    out, done, failed = B.host_group_reduce(rec, 4, leave_shard=leave_shard, leave_after=leave_after, timeout_s=60.0)
    q.put((out, done, failed))


@pytest.mark.parametrize("S,leave_shard,leave_after", [(2, 1, 0), (3, 0, 5), (8, 7, 11)])
def test_a_shard_that_leaves_makes_the_others_return(S, leave_shard, leave_after):
    """one thread leaves after `leave_after` rounds: every other thread comes back with an error at its next round instead
    of waiting (in a child with a timeout: a deadlock fails this test, it does not hold up the suite)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_abandon_child, args=(q, S, leave_shard, leave_after))
    p.start()
    try:
        out, done, failed = q.get(timeout=30)                # far below the group's own 60 s limit: leave() woke them
        p.join(timeout=30)
    finally:
        if p.is_alive():                                     # a deadlocked child must not stay behind
            p.kill()
            p.join()
    assert p.exitcode == 0
    rec = _records(S, 12, 4, 2, seed=11)
    exp = _shard_order(rec, 4)
    for s in range(S):
        assert done[s] == leave_after
        assert failed[s] == (0 if s == leave_shard else 1)
        assert np.array_equal(out[s, :leave_after], exp[:leave_after])       # the rounds before it are whole


def test_stand_alone_group_check_builds_and_passes(tmp_path):
    """tests/c_harness/shard_group_check.cpp: reduce / reduce_vec of the group from 1, 2, 3 and 8 threads against a serial
    rank-order sum, bit for bit, with a shard that leaves mid-way -- shard_group.hpp alone, no HIP, no library.  (The
    same program is what the thread and address sanitizers are pointed at; here it is built plain.)"""
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "shard_group_check"
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "shard_group_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4, r.stdout


def test_stand_alone_block_pool_check_builds_and_passes(tmp_path):
    """tests/c_harness/block_pool_check.cpp: the job pool of the concurrent block projections with 1, 2 and 8 threads --
    every listed index runs exactly once per call, a job's first error is rethrown after the call's other jobs ran, the
    pool serves the next call and is destroyed with idle workers -- block_pool.hpp alone, no HIP, no library.  (The same
    program is what the thread and address sanitizers are pointed at; here it is built plain.)"""
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "block_pool_check"
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "block_pool_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3, r.stdout
