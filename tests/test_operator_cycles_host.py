"""CPU checks of the operator-form per-cycle tests (operator_cycle_cases.py): every case's fp64 reference run has not converged
before its last captured cycle and stays below 32 x 2^-52 sqrt(K) in every quantity (no bound of the GPU test is vacuous), the
row patterns are the prescribed ones, the operator built from the support list's definition agrees with the dense matrix smat
gives, deliberately wrong operators fail the GPU test's own rule at MARGIN, the binding mirrors the header's struct and the entry
refuses invalid arguments before it touches a device."""
import ctypes
import math
import re

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd.state_io import smat

import lanczos_cycle_cases as L
import operator_cycle_cases as O


def _distinct(cases):
    seen, out = set(), []
    for cs in cases:
        key = (cs["n"], cs["nev"], cs["kd"], cs["rp"], cs["pattern"], cs["no_factors"], cs["opts"].get("eigsolver", 2))
        if key not in seen:
            seen.add(key)
            out.append(cs)
    return out


def _all_cases():
    l2 = O.l2_case()
    return O.CASES + ([l2] if l2 is not None else [])


RUNS = _distinct(_all_cases())


def test_the_table_reaches_every_branch():
    cases = _all_cases()
    assert {c["engine"] for c in cases} == {"step", "block1"}
    assert all(c["kd"] == max(2 * c["nev"] + 1, c["opts"]["eigsolver_min_lanczos"]) <= 255 for c in cases)
    by = lambda **kw: [c for c in cases if all(c[k] == v for k, v in kw.items())]
    # k_fop / k_fop_finish <1 | 2, OWN> and k_lz_orth<., 1 | 2, OWN>
    for nchp in (1, 2):
        for owner in (False, True):
            assert by(engine="step", nchp=nchp, owner=owner), (nchp, owner)
    assert {c["rp"] for c in by(n=257) if c["opts"].get("eigsolver", 2) == 2} == {63, 64, 65, 127}
    assert {(c["rp"], c["owner"]) for c in by(n=400)} == {(7, True), (8, True), (14, True), (15, False)}
    assert by(n=2100, rp=66, owner=True, nchp=2)
    # pld > 64: both chunk counts and the second form; the second form below it; keep > 64; dsaupd; a factor offset
    assert {(c["rp"], c["no_factors"]) for c in by(n=4097)} == {(3, False), (65, False), (0, True)}
    assert by(n=129, no_factors=True) and by(n=300, no_factors=True)
    assert any((3 * c["kd"]) // 5 > 64 and c["rp"] > 64 for c in cases)
    assert any(c["opts"].get("eigsolver") == 1 and c["f_first"] > 0 for c in cases)
    # the one-workgroup kernel: E in LDS, its factor limit from both sides, its refusal of overflow rows
    assert by(n=129, rp=16, engine="block1", ell_in_lds=True) and by(n=129, rp=17, engine="step")
    lds = {O.expect_ell_in_lds(c, O.operator(c)[0]) for c in by(engine="block1")}
    assert lds == {True, False}
    assert any(c["overflow_rows"] > 0 and c["opts"].get("lanczos_cycle_kernel") == 2 and c["engine"] == "step" for c in cases)
    assert by(ell_w=1) and by(pattern="rounds", engine="step") and by(pattern="rounds", engine="block1")
    assert len(O.WARM_CASES) == 2 and len(O.PROBE_CASES) == 2 and len(O.OWNER_CASES) >= 4


def test_block1_reads_a_wide_e_through_l2_at_some_legal_side():
    """b1_lds_plan (through its host entry): without E every nt <= 8 fits the 160 KiB of a workgroup, with a 32-wide E in LDS
    the plan outgrows them from some nt on -- the case that runs k_lz_block1<., true> with ell_in_lds = 0"""
    assert all(8 * B.block1_lds_doubles(nt, True, 0, 0) <= 160 * 1024 for nt in range(1, 9))
    cs = O.l2_case()
    assert cs is not None and 64 * 2 < cs["n"] <= 64 * 8
    nt = (cs["n"] + 63) // 64
    assert 8 * B.block1_lds_doubles(nt, True, 0, 32) > 160 * 1024 >= 8 * B.block1_lds_doubles(nt - 1, True, 0, 32)
    assert 8 * B.block1_lds_doubles(3, True, 0, 10) <= 160 * 1024          # (n = 129, rank 16, the sparse pattern: E in LDS)
    with pytest.raises(ValueError):
        B.block1_lds_doubles(9, True)


def test_row_patterns_are_the_prescribed_ones():
    rng = np.random.default_rng(0)
    cnt = O.Operator(64, O.pattern_diag(64, rng), np.ones(64), np.zeros((64, 0)), np.zeros(0)).row_counts()
    assert np.all(cnt == 1)
    s = O.pattern_rounds(130, rng)
    cnt = O.Operator(130, s, np.ones(len(s)), np.zeros((130, 0)), np.zeros(0)).row_counts()
    assert all(cnt[r] == c for r, c in O.ROUNDS.items()) and cnt[O.ROUNDS_EMPTY] == 0 and cnt.max() == 32
    s = O.pattern_overflow(330, rng)
    cnt = O.Operator(330, s, np.ones(len(s)), np.zeros((330, 0)), np.zeros(0)).row_counts()
    assert cnt[O.OVER_33] == 33 and cnt[O.OVER_HUB] == 300 > 32 + 256 and cnt[O.OVER_WIDE] == 40 and cnt[329] == 40
    assert O.OVER_HUB // 64 == O.OVER_WIDE // 64 and 329 // 64 == 5 and int((cnt > 32).sum()) == 4
    cs = O.l2_case()
    s = O.cs_pieces(cs)[0]
    cnt = O.Operator(cs["n"], s, np.ones(len(s)), np.zeros((cs["n"], 0)), np.zeros(0)).row_counts()
    assert cnt.max() == 32
    for cs in O.CASES:
        if cs["pattern"] == "sparse":
            assert 1 <= O.operator(cs)[0].row_counts().max() <= 32


@pytest.mark.parametrize("cs", [c for c in RUNS if c["n"] <= 330], ids=lambda c: c["id"])
def test_operator_agrees_with_the_dense_matrix(cs):
    """the support list's definition against smat of the packed vector that holds the values: the same matrix; both mat-vecs of
    the operator against the dense products"""
    n = cs["n"]
    A, normA = O.operator(cs)
    packed = np.zeros(n * (n + 1) // 2)
    packed[A.support] = A.values
    D = smat(packed, n) + (A.F * A.lam) @ A.F.T
    assert np.abs(A.dense() - D).max() <= 4 * L.EPS * normA and np.array_equal(A.dense_e(), A.dense_e().T)
    assert np.abs(np.linalg.eigvalsh(A.dense_e())).max() <= (1.0 if not cs["no_factors"] else 12.5) + 1e-12
    if cs["rp"] > 0:
        assert np.abs(A.F.T @ A.F - np.eye(cs["rp"])).max() <= 64 * L.EPS
    rng = np.random.default_rng(5)
    V = rng.standard_normal((n, 3))
    for c in range(3):
        assert np.abs(A @ V[:, c] - D @ V[:, c]).max() <= 64 * L.EPS * normA * np.abs(V[:, c]).max() * math.sqrt(n)
    assert float(np.abs(A.times_ld(V) - D.astype(L.LD) @ V.astype(L.LD)).max()) <= 64 * L.EPS * normA * np.abs(V).max() * math.sqrt(n)


@pytest.mark.parametrize("cs", RUNS, ids=lambda c: c["id"])
def test_reference_has_not_converged_early_and_is_accurate(cs):
    """the CPU side of the GPU test's conditions: the fp64 reference run on the operator has not converged before the last
    captured cycle, and its own R1 - R3 stay below HOST_BOUND sqrt(K)"""
    A, normA = O.operator(cs)
    run, early = O.reference_cycles(cs)
    assert not early and len(run) == cs["cycles"]
    reuse = None
    for c, cyc in enumerate(run):
        q, reuse = L.quantities(A, normA, cyc, reuse)
        assert (cyc["kfirst"] == 0) == (c == 0) and q["beta_min"] > 0.0
        for name in L.QUANTITIES:
            assert q[name] <= L.HOST_BOUND * math.sqrt(cyc["K"]), (c, name, q[name])


def _case(n, rp, pattern, no_factors=False):
    return next(c for c in O.CASES if (c["n"], c["rp"], c["pattern"], c["no_factors"]) == (n, rp, pattern, no_factors))


@pytest.mark.parametrize("variant,cs", [("drop_overflow", _case(330, 6, "overflow")), ("no_sqrt2", _case(130, 6, "rounds")),
                                        ("no_mirror", _case(130, 6, "rounds")), ("lam64", _case(257, 65, "sparse")),
                                        ("other_half", _case(129, 0, "sparse", True))], ids=lambda p: p if isinstance(p, str) else p["id"])
def test_wrong_operators_fail_the_rule_of_the_gpu_test(variant, cs):
    """a cycle run on a wrong operator, judged as the GPU test judges a kernel's: its quantities under the TRUE operator against
    the plain reference cycle from the same inputs, with the same margin and floor.  One wrong entry of E, one factor column
    left out or the other half of the support-value array all break the Krylov-Schur relation of the first cycle."""
    A, normA = O.operator(cs)
    Aw, _ = O.operator(cs, variant)
    arpack = cs["opts"].get("eigsolver", 2) == 1
    run, _ = L.reference_run(Aw, L.start(cs["n"]), cs["nev"], cs["kd"], 1, arpack=arpack)
    cyc = run[0]
    Vr, alr, ber = L.reference_cycle(A, cyc["V"], cyc["kfirst"], cyc["K"])
    qw, reuse = L.quantities(A, normA, cyc)
    qr, _ = L.quantities(A, normA, dict(cyc, V=Vr, alphas=alr, betas=ber), reuse)
    flagged = {name for name in L.QUANTITIES if qw[name] > L.bound(qr[name])}
    assert {"r1_all", "r1_own"} <= flagged, (flagged, qw, qr)
    # ... and the unchanged operator passes it
    run, _ = L.reference_run(A, L.start(cs["n"]), cs["nev"], cs["kd"], 1, arpack=arpack)
    qk, _ = L.quantities(A, normA, run[0])
    assert all(qk[name] <= L.bound(qr[name]) for name in L.QUANTITIES)


def test_rank5_pieces_are_exact():
    support, values, other, F, lam, normA = O.rank5_pieces(130)
    A = O.Operator(130, support, values, F, lam)
    assert np.array_equal(A.dense(), L.rank5_matrix(130)[0]) and np.all(values == 0.0) and len(support) == 130
    V, al, be = L.reference_cycle(A, L.start(130)[:, None] * np.ones((1, 31)), 0, 6)
    assert be[5] <= L.TOL and np.all(be[:5] > 1e-3)


def test_ev_bound_flags_a_wrong_row():
    cs = _case(130, 6, "rounds")
    A, _ = O.operator(cs)
    v = L.start(130)
    i, j = O.unpacked_index(A.support)
    e = np.where(i == j, A.values, A.values * 0.70710678118654752440)      # (the product form: one rounding, as the bound counts)
    off = i != j
    ev = np.bincount(np.concatenate([i, j[off]]), weights=np.concatenate([e * v[j], (e * v[i])[off]]), minlength=130)
    assert O.ev_rows_within_bound(A, v, ev) == [] and ev[O.ROUNDS_EMPTY] == 0.0
    wrong = ev.copy()
    wrong[77] *= 1.0 + 1e-13
    wrong[O.ROUNDS_EMPTY] = -0.0
    assert [b[0] for b in O.ev_rows_within_bound(A, v, wrong)] == [O.ROUNDS_EMPTY, 77]


def _named(header, name):
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", header, re.S)
    return "typedef struct " + name + " {" + m.group(1) + "} " + name + ";"


def test_binding_exposes_the_entry_and_mirrors_the_struct():
    assert B.lib().proxsdp_hip_abi_version() == 10
    for name in ("proxsdp_hip_operator_cycles", "proxsdp_host_block1_lds_doubles"):
        assert name in set(B.header_symbols()) and hasattr(B.lib(), name)
    import test_host_abi as T
    header = B.HEADER_PATH.read_text()
    name = "proxsdp_operator_cycles"
    assert [f for f, _ in B.OperatorCyclesIO._fields_] == T._c_struct_fields(_named(header, name), name)
    # every member is 4 or 8 bytes wide and the 4-byte ones come in pairs: no padding, the size is the sum
    assert ctypes.sizeof(B.OperatorCyclesIO) == 8 + 4 * 8 + 8 + 8 * 7 + 8 + 8 * 9 + 4 * 6 == 208
    assert int(re.search(r"#define PROXSDP_OP_INFO\s+(\d+)", header).group(1)) == B.OP_INFO == 16


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """code -1 with or without a GPU; a valid call without one fails loudly with -2"""
    n = 10
    N = n * (n + 1) // 2
    supp = O.pattern_diag(n, None)
    vals = np.ones(n)
    F = np.linalg.qr(np.random.default_rng(0).standard_normal((n, 2)))[0]
    lam = np.array([3.0, 2.0])

    def refused(match, support=supp, values=vals, F=F, lam=lam, nev=2, max_cycles=2, n=n, opts=None, **kw):
        o = B.default_options()
        for k, v in dict(dict(eigsolver_min_lanczos=5), **(opts or {})).items():
            B.set_option(o, k, v)
        with pytest.raises(B.ProxSDPHipError, match=match) as e:
            B.operator_cycles(n, support, values, F, lam, nev, max_cycles, options=o, **kw)
        assert e.value.code == -1

    refused("n must be", n=1, support=[0], values=[1.0], F=np.zeros((1, 0)), lam=[], nev=1)
    refused("nev must be", nev=0)
    refused("nev must be", nev=11)
    refused("max_cycles < 1", max_cycles=0)
    refused("at most 255", opts=dict(eigsolver_min_lanczos=256))
    refused("another driver", opts=dict(krylovkit_eager=1))
    refused("switches the operator form off", opts=dict(lanczos_operator=0))
    refused("rp must be", F=np.zeros((n, 11)), lam=np.ones(11))
    refused("f_first must be", f_first=128)
    refused("f_first must be", f_first=-1)
    refused("the second form has no factors", no_factors=True)
    refused("strictly ascending", support=[0, 2, 2], values=[1.0, 1.0, 1.0])
    refused("strictly ascending", support=[5, 3], values=[1.0, 1.0])
    refused("strictly ascending", support=[0, N], values=[1.0, 1.0])
    refused("strictly ascending", support=[-1, 3], values=[1.0, 1.0])
    refused("support value is not finite", values=np.where(np.arange(n) == 4, np.inf, 1.0))
    refused("factor entry is not finite", F=np.where(np.arange(2 * n).reshape(n, 2) == 7, np.nan, F))
    refused("factor entry is not finite", lam=[3.0, np.inf])
    refused("lam must be positive", lam=[3.0, 0.0])
    refused("vector entry is not finite", resid=np.where(np.arange(n) == 1, np.nan, 1.0))
    refused("vector entry is not finite", probe_v=np.where(np.arange(n) == 1, np.inf, 1.0))
    big = 130
    with pytest.raises(B.ProxSDPHipError, match="rp must be") as e:
        B.operator_cycles(big, O.pattern_diag(big, None), np.ones(big), np.zeros((big, 128)), np.ones(128), 2, 2)
    assert e.value.code == -1
    if B.device_count() <= 0:
        o = B.default_options()
        B.set_option(o, "eigsolver_min_lanczos", 5)
        with pytest.raises(B.ProxSDPHipError) as e:
            B.operator_cycles(n, supp, vals, F, lam, 2, 2, options=o)
        assert e.value.code == -2
