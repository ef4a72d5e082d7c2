"""CPU checks of the positive-part tests (positive_part_cases.py): the dimensions and kernel instantiations the case tables reach,
the fp64 reference run of every run case (it restarts, needs the stated cycles and returns the constructed count; the failure
exits fail), the reference certificate on the exact case list (must-pass spectra pass with theta_max in [-0.61, -0.50], a hidden 7
is found to four digits, every must-fail case fails), `rule` on hand-made (D, f), the long-double pieces against fp64, the
binding's struct against the header and the entry's refusals before a device is touched."""
import ctypes
import re

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import lanczos_cycle_cases as L
import operator_cycle_cases as O
import positive_part_cases as P


def test_dimensions_and_the_instantiations_the_tables_reach():
    o = B.default_options()
    assert (B.get_option(o, "eigsolver_min_lanczos"), B.get_option(o, "full_eig_lanczos_kdim10")) == (P.MIN_LANCZOS, P.KDIM10)
    assert (B.get_option(o, "krylovkit_tol"), B.get_option(o, "full_eig_lanczos_posres")) == (P.TOL, P.POSRES)
    assert 1e-2 * min(B.get_option(o, k) for k in ("tol_gap", "tol_feasibility", "tol_primal", "tol_dual")) >= P.POSRES
    for cs in P.RUN_CASES:
        assert B.positive_part_dims(cs["n"], cs["nev"], cs["ws_rank"]) == (cs["cap"], cs["kd"]) == P.dims(cs["n"], cs["nev"], cs["ws_rank"])
    assert [c["kd"] for c in P.RUN_CASES] == [29, 29, 29, 128, 218, 41]
    assert {P.nch(c["kd"]) for c in P.RUN_CASES} == {1, 2, 4} and P.nch(128 + 1) == 3          # (the restart's 129-column basis)
    clipped = P.RUN_CASES[-1]
    assert clipped["kd"] == clipped["cap"] - 1 < max(2 * clipped["nev"] + 1, 3 * clipped["nev"] + 8)
    assert {c["engine"] for c in P.RUN_CASES} == {"step", "block1"}
    # the certificate: k_lz_measure<1 | 2>, npos = 0 (k_lz_begin), a run across 64 and across 128 columns, both forms
    packed = [c for c in P.CERT_CASES if c["form"] == "packed"]
    assert {c["npos"] for c in packed if c["steps"] == 10 and c["kind"] == "clean" and c["n"] == 257} == set(P.NPOS)
    assert {c["npos"] for c in packed if c["steps"] == 10 and c["kind"] == "clean" and c["n"] == 130} == set(P.NPOS)
    assert {P.nch(c["npos"]) for c in P.CERT_CASES if c["npos"] > 0} == {1, 2}
    assert {c["steps"] for c in packed} == {2, 10, 30}
    assert any(c["npos"] < 64 < c["npos"] + c["steps"] for c in packed) and any(c["npos"] < 128 < c["npos"] + c["steps"] for c in packed)
    op = [c for c in P.CERT_CASES if c["form"] == "operator"]
    assert {c["npos"] for c in op if c["kind"] == "clean"} == {0, 17, 60, 65}
    assert any(c["rp"] <= 64 for c in op) and any(c["rp"] > 64 for c in op)
    assert any(O.owner_rule(c["n"], c["rp"], "step") for c in op) and any(not O.owner_rule(c["n"], c["rp"], "step") for c in op)
    assert all(c["npos"] + c["steps"] + 1 <= P.dims(c["n"], c["nev"], c["ws_rank"])[0] for c in P.CERT_CASES + [P.SMALL_COMPLEMENT])
    assert P.TOO_SMALL["npos"] + P.TOO_SMALL["steps"] + 1 > P.dims(130, 7, P.TOO_SMALL["ws_rank"])[0] == 42
    # the warm start: one and two chunks of factor columns, the LDS table's last entries, every weight rule
    assert {c["rp"] for c in P.WARM_CASES} == {1, 5, 64, 65, 127} and {c["f_first"] for c in P.WARM_CASES} == {0, 40}
    assert {c["wpow"] for c in P.WARM_CASES} == {1.0, 0.5, 0.0} and {c["lam_kind"] for c in P.WARM_CASES} == {"plain", "small", "denormal"}
    assert any(c["warm"] < 0 for c in P.WARM_CASES)


@pytest.mark.parametrize("cs", P.RUN_CASES + P.TOL_CASES, ids=lambda c: c["id"])
def test_reference_run_restarts_and_returns_the_constructed_count(cs):
    A, _, normA, _, ev = P.run_matrix(cs)
    assert int((ev > 0).sum()) == cs["npos"] <= cs["nev"] and np.abs(ev).min() >= 1e-3 * normA
    cyc, dec = P.reference_run(A, P.run_start(cs), cs["nev"], cs["kd"], P.MAX_CYCLES, tol_rel=cs.get("tol_rel", 0.0))
    assert dec["decision"] == "accept" and dec["count"] == cs["npos"]
    assert len(cyc) == cs["cycles"] and (len(cyc) >= 2 or cs is P.TOL9_CASE)
    if cs["tight"]:
        # the positive pairs' tolerance decides the first cycle: krylovkit_tol goes on, 1e-9 x scale accepts
        D, _, f = P.rayleigh(cyc[0])
        assert P.rule(D, f, cs["nev"], P.TOL, P.POSRES)["decision"] == "go_on"
        assert P.rule(D, f, cs["nev"], P.TOL, P.POSRES, tol_rel=1e-9)["decision"] == "accept"
        assert P.TOL < np.abs(f[:cs["npos"]]).max() < 1e-10 and abs(f[cs["npos"]]) < P.POSRES
    for c in cyc:
        q, _ = L.quantities(A, normA, c)
        assert all(q[k] <= L.HOST_BOUND * np.sqrt(c["K"]) for k in L.QUANTITIES), q


def test_reference_run_takes_the_failure_exits():
    cs = P.TOO_MANY
    A, _, _, _, _ = P.run_matrix(cs)
    cyc, dec = P.reference_run(A, L.start(cs["n"]), cs["nev"], cs["kd"], P.MAX_CYCLES)
    assert len(cyc) == 1 and dec["decision"] == "too_many" and dec["count"] > cs["nev"]
    cs = P.MAXITER
    A, _, _, _, _ = P.run_matrix(cs)
    cyc, dec = P.reference_run(A, L.start(cs["n"]), cs["nev"], cs["kd"], 1)
    assert len(cyc) == 1 and dec["decision"] == "maxiter"


@pytest.mark.parametrize("cs", P.CERT_CASES + [P.SMALL_COMPLEMENT], ids=lambda c: c["id"])
def test_reference_certificate_meets_the_case_conditions(cs):
    n, npos, m = cs["n"], cs["npos"], cs["steps"]
    A, _, normA, Z, vals = P.cert_inputs(cs)
    r2 = P.resid2(n)
    assert abs(np.linalg.norm(r2) - 1.0) <= 8 * P.EPS
    cos = abs(float(r2 @ L.start(n)))
    assert cos < 0.5, cos
    assert npos == 0 or np.abs(Z.T @ Z - np.eye(npos)).max() <= 64 * P.EPS
    ref = P.certificate_reference(A, Z, vals, r2, m)
    theta = ref["theta_max"]
    al, be = ref["alphas"][npos:npos + ref["steps"]], ref["betas"][npos:npos + ref["steps"]]
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    scale = P.cert_scale(theta, np.linalg.eigvalsh(T)[0], vals)
    top = P.complement_max(A, Z)
    assert theta <= top + 1e-13 * m * normA
    if cs is P.SMALL_COMPLEMENT:
        assert not P.decision(theta, scale)
        return
    assert ref["steps"] == m and np.all(be > 0.0)
    assert P.decision(theta, scale) == cs["must_pass"], (theta, scale)
    if cs["kind"] == "clean":
        assert top <= (-0.5 if cs["form"] == "packed" else -0.2)
        if cs["form"] == "packed" and m == P.STEPS:
            # ([-0.61, -0.50] where the largest remaining eigenvalue is the bulk's edge -0.5; 30 remaining values end lower)
            assert P.CLEAN[0] - P.CLEAN[1] <= theta - top <= 1e-13 * m * normA and theta <= P.CLEAN[1], (theta, top)
            assert top < -0.51 or P.CLEAN[0] <= theta, (theta, top)
    elif cs["kind"] == "hidden7":
        assert abs(theta - 7.0) <= P.HIDDEN7, theta
    else:
        assert top >= 1.0 - 64 * P.EPS and theta > 1e-3 * scale
    # the long-double recurrence from the same vector agrees: what the GPU test measures against is no artefact
    rl = P.certificate_reference(A, Z, vals, r2, m, dtype=P.LD)
    assert abs(float(rl["theta_max"]) - theta) <= 1e-13 * m * normA
    assert float(np.abs(rl["V"][:, npos].astype(np.float64) - ref["V"][:, npos]).max()) <= 64 * P.EPS


def test_reference_on_the_hazard_of_the_certified_projection():
    A, _, lam, deficient, nev = P.hazard()
    n = A.shape[0]
    cap, kd = P.dims(n, nev, 127)
    cyc, dec = P.reference_run(A, deficient, nev, kd, P.MAX_CYCLES)
    assert dec["decision"] == "accept" and dec["count"] == 4 == int((lam > 0).sum()) - 3
    D, U, _ = P.rayleigh(cyc[-1])
    Z = cyc[-1]["V"][:, :kd] @ U[:, :4]
    assert np.abs(np.sort(D[:4]) - np.array([1.0, 3.0, 5.0, 9.0])).max() <= 1e-9
    ref = P.certificate_reference(A, Z, D[:4], P.resid2(n), P.STEPS)
    assert abs(ref["theta_max"] - 7.0) <= P.HIDDEN7 and not P.decision(ref["theta_max"], 9.0)


def test_rule_on_hand_made_ritz_pairs():
    tol, posres = 1e-12, 1e-6
    D = np.array([9.0, 4.0, 1.0, -0.5, -2.0, -3.0])
    f = np.array([1e-14, 1e-13, 5e-13, 2e-6, 0.3, 0.4])
    r = P.rule(D, f, 5, tol, posres)
    assert (r["decision"], r["count"], r["converged"], r["jn"], r["scale"]) == ("accept", 3, 3, 3, 9.0)
    assert r["tol_neg"] == 9e-6 and r["tol_pos"] == tol
    assert P.rule(D, np.where(np.arange(6) == 3, 1e-5, f), 5, tol, posres)["decision"] == "go_on"       # the negative pair above 9e-6
    assert P.rule(D, np.where(np.arange(6) == 2, 2e-12, f), 5, tol, posres)["decision"] == "go_on"      # a positive pair above tol
    assert P.rule(D, np.where(np.arange(6) == 2, 2e-12, f), 5, tol, posres, tol_rel=1e-9)["decision"] == "accept"
    assert P.rule(D, f, 3, tol, posres)["decision"] == "accept" and P.rule(D, f, 2, tol, posres)["decision"] == "too_many"
    # a residual merely below |theta| is not enough; an exactly-zero pair is skipped: the pair behind it decides
    Dz = np.array([9.0, 1.0, 0.0, -1e-13 * 9.0, -0.5, -3.0])
    fz = np.array([0.0, 0.0, 0.0, 0.3, 1e-7, 0.4])
    rz = P.rule(Dz, fz, 4, tol, posres)
    assert (rz["decision"], rz["count"], rz["jn"]) == ("accept", 2, 4)
    assert P.rule(Dz, np.where(np.arange(6) == 4, 0.4, fz), 4, tol, posres)["decision"] == "go_on"
    # every Ritz value positive: nothing negative to resolve
    assert P.rule(np.array([3.0, 2.0]), np.array([1e-13, 1e-13]), 2, tol, posres)["decision"] == "accept"
    # no positive value: the first pair decides, whatever the rest
    assert P.rule(np.array([-0.5, -1.0]), np.array([1e-7, 0.5]), 2, tol, posres) == dict(
        count=0, converged=0, jn=0, scale=1.0, tol_pos=tol, tol_neg=1e-6, decision="accept")


def test_long_double_pieces_agree_with_fp64():
    rng = np.random.default_rng(3)
    al, be = rng.standard_normal(12), np.abs(rng.standard_normal(12)) + 0.1
    assert abs(float(P.tridiag_max(al, be, P.LD)) - P.tridiag_max(al, be)) <= 1e-14 * 12
    lam = np.array([9.0, 3.0, 9e-9, 1e-310, 1.0])
    w = P.warm_weights(lam, 1.0)
    assert np.array_equal(w, [1.0, 3.0, 1e6, 1e6, 9.0]) and np.all(P.warm_weights(lam, 0.0) == 1.0)
    assert np.allclose(P.warm_weights(lam, 0.5), np.sqrt(w), rtol=1e-15)
    assert np.abs(P.warm_weights(lam, 0.5, P.LD).astype(np.float64) - np.sqrt(w)).max() <= 2e-13


def _named(header, name):
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", header, re.S)
    return "typedef struct " + name + " {" + m.group(1) + "} " + name + ";"


def test_binding_exposes_the_entry_and_mirrors_the_struct():
    assert "proxsdp_hip_positive_part" in set(B.header_symbols()) and hasattr(B.lib(), "proxsdp_hip_positive_part")
    import test_host_abi as T
    header = B.HEADER_PATH.read_text()
    name = "proxsdp_positive_part"
    assert [f for f, _ in B.PositivePartIO._fields_] == T._c_struct_fields(_named(header, name), name)


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """code -1 with or without a GPU; a valid call without one fails loudly with -2"""
    n = 10
    A, packed, _, Q, ev = P.spectrum(n, 2)
    op = dict(support=O.pattern_diag(n, None), values=-np.ones(n), F=Q[:, :2], lam=np.array([3.0, 2.0]))

    def refused(match, nev=2, ws_rank=4, max_cycles=2, opts=None, block=None, **kw):
        o = B.default_options()
        for k, v in (opts or {}).items():
            B.set_option(o, k, v)
        with pytest.raises(B.ProxSDPHipError, match=match) as e:
            B.positive_part(n, nev, ws_rank, max_cycles, options=o, **(block or dict(packed=packed)), **kw)
        assert e.value.code == -1

    # what the wrapped entries refuse
    refused("nev must be", nev=0)
    refused("max_cycles < 1", max_cycles=0)
    refused("another driver", opts=dict(krylovkit_eager=1))
    refused("switches the operator form off", block=dict(operator=op), opts=dict(lanczos_operator=0))
    refused("lam must be positive", block=dict(operator=dict(op, lam=np.array([3.0, 0.0]))))
    refused("vector entry is not finite", block=dict(operator=op), resid=np.where(np.arange(n) == 1, np.nan, 1.0))
    # its own
    refused("never takes the positive-part run", opts=dict(eigsolver=1))
    refused("ws_rank < 1", ws_rank=0)
    refused("no run needs a locked set", run=False, cert_steps=10)
    refused("npos_in must be", run=False, cert_steps=2, locked=np.zeros((n, n + 1)), locked_vals=np.zeros(n + 1))
    refused("locked entry is not finite", run=False, cert_steps=2, locked=np.where(np.arange(2 * n).reshape(n, 2) == 3, np.inf, Q[:, :2]),
            locked_vals=ev[:2])
    refused("locked value is not finite", run=False, cert_steps=2, locked=Q[:, :2], locked_vals=np.array([9.0, np.nan]))
    refused("cert_steps out of range", cert_steps=-1)
    # a stated dimension that is not the positive-part run's, a stated cap that is not the workspace's
    t = B.LanczosCyclesIO()
    cap, kd = B.positive_part_dims(n, 2, 4)
    assert (cap, kd) == (26, 25)
    for bad_cols, bad_cap, match in ((kd, cap, "cols must be"), (kd + 1, cap + 1, "cap must be")):
        p = B.PositivePartIO()
        p.struct_size = ctypes.sizeof(B.PositivePartIO)
        t.struct_size = ctypes.sizeof(B.LanczosCyclesIO)
        t.n, t.nev, t.max_cycles, t.cols, t.ldv = n, 2, 1, bad_cols, 64
        x = np.ascontiguousarray(packed)
        info = np.zeros(B.LZ_INFO, dtype=np.int32)
        V, z = np.zeros(64 * (kd + 1)), [np.zeros(kd + 1) for _ in range(4)]
        t.packed, t.info, t.V = B._p(x), B._p(info, B.pi32), B._p(V)
        t.alphas, t.betas, t.D, t.f = (B._p(a) for a in z)
        bufs = [np.zeros(bad_cap) for _ in range(3)] + [np.zeros(bad_cap * 64) for _ in range(2)] + [np.zeros(64)]
        p.vals, p.cert_alphas, p.cert_betas, p.Z, p.basis, p.resid2 = (B._p(a) for a in bufs)
        p.packed_run, p.ws_rank, p.cap, p.run, p.npos_in = ctypes.pointer(t), 4, bad_cap, 1, -1
        assert B.lib().proxsdp_hip_positive_part(ctypes.byref(p)) == -1
        assert match in B.lib().proxsdp_hip_last_error().decode()
    p.packed_run = None
    assert B.lib().proxsdp_hip_positive_part(ctypes.byref(p)) == -1 and "one of packed_run" in B.lib().proxsdp_hip_last_error().decode()
    # the Krylov branch's dimension limit is not the positive-part run's (2 nev + 1 = 261 is clipped to cap - 1 = 255): the packed
    # entry itself refuses the same nev without the wide workspace
    big = 140
    _, pbig, _, _, _ = P.spectrum(big, 2)
    assert B.positive_part_dims(big, 130, 127) == (256, 255)
    with pytest.raises(B.ProxSDPHipError, match="needs the wide workspace") as e:
        B.lanczos_cycles(pbig, big, 130, 1)
    assert e.value.code == -1
    if B.device_count() <= 0:
        for args in ((n, 2, 4, 2, packed), (big, 130, 127, 1, pbig)):
            with pytest.raises(B.ProxSDPHipError) as e:
                B.positive_part(*args[:4], packed=args[4])
            assert e.value.code == -2
