"""Every cycle of the production Lanczos driver on the OPERATOR FORM against exact checks (proxsdp_hip_operator_cycles:
Solver::lanczos with its per-cycle observer installed, the block given by a support list, its values and the previous
projection's factors; the ELL / overflow layout is built by setup_support's own code).

  step kernels    k_fop<1 | 2, OWN>, k_fop_finish<1 | 2, NCH, OWN> (fop_body: the prefetched first round of 16 ELL entries a row
                  and the later ones, the overflow list, the stop early-out; fop_owner_body), k_lz_orth<NCH, 1 | 2, OWN> with
                  pld <= 64 and pld > 64, NCH = 1 .. 3
  block1          k_lz_block1<., true> with E in LDS and read through L2; its refusals (factor rank above 16, an overflow row)
  warm start      k_lz_warm_sum / k_lz_warm_scale

The rule is test_lanczos_cycles.py's, unchanged: per captured cycle, in long double (lanczos_cycle_cases.quantities on
operator_cycle_cases.Operator: A V = F (lam o (F' V)) + E V from the support list's definition), R1 - R3 and beta > 0; a quantity
may be MARGIN = 8 times what the plain fp64 reference cycle gives from the SAME cycle's inputs, floor 8 x 2^-52; the exact
hand-over checks (padding rows, start column, v_kfirst, the kept columns' repeat).  Each case names the engine lz_plan must choose
and what every cycle must report: mat-vecs on the operator-form kernels, owner or records form, the chunks of factor columns, the
ELL width, the overflow rows, for block1 whether E sat in LDS.

block1 against step: test_lanczos_cycles.py ties the two engines by nothing but the rule above (profiles/lanczos_cycles.md shows
equal digits, no test asserts equal bits), so here too each engine stands on its own checks.

Not reached here: the lam-power weights of k_lz_warm_sum (positive-part runs only; the entry runs the Krylov branch's lanczos()).
They, the positive-part run and its certificate on the operator form are test_positive_part.py's."""
from fractions import Fraction

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import lanczos_cycle_cases as L
import operator_cycle_cases as O

pytestmark = pytest.mark.gpu


def _positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


def _cases():
    l2 = O.l2_case()
    return O.CASES + ([l2] if l2 is not None else [])


def _reports(cs, A, got, cy):
    """what the plan and the layout must report for the case"""
    cnt = A.row_counts()
    ell_w, over = min(max(int(cnt.max()), 1), 32), int((cnt > 32).sum())
    assert cs["ell_w"] in (None, ell_w) and cs["overflow_rows"] == over
    assert (got["ell_w"], got["overflow_rows"]) == (ell_w, over)
    assert cy["engine"] == cs["engine"], (cy["engine"], cs["engine"])
    assert cy["fop"] == cy["K"] - cy["kfirst"] > 0, "the cycle's mat-vecs ran on the operator-form kernels"
    assert cy["owner"] == cs["owner"] and cy["nchp"] == cs["nchp"]
    assert (cy["ell_w"], cy["overflow_rows"]) == (ell_w, over)
    assert cy["ell_in_lds"] == O.expect_ell_in_lds(cs, A)


@pytest.mark.parametrize("cs", _cases(), ids=lambda c: c["id"])
def test_every_cycle_is_a_krylov_schur_decomposition(cs):
    n, kd = cs["n"], cs["kd"]
    A, normA = O.operator(cs)
    got = O.capture(cs)
    cyc = got["cycles"]
    assert got["krylovdim"] == kd and got["npad"] == 64 * ((n + 63) // 64)
    # conditions: the cycles asked for were captured, every one on the operator-form kernels
    assert len(cyc) == cs["cycles"], (len(cyc), cs["cycles"])
    assert got["untouched"]["info"].size == 0
    v0 = L.start(n)
    failures, prev, reuse = [], None, None
    for c, cy in enumerate(cyc):
        K, kf, V = cy["K"], cy["kfirst"], cy["V"]
        _reports(cs, A, got, cy)
        assert cy["stop"] == 0 and K == kd
        assert (kf == 0) == (c == 0) and 0 <= kf < K
        # ---- hand-over, exact
        assert _positive_zero(V[n:, :K + 1]), "padding rows"
        assert np.all(cy["alphas"][:kf] == B.SYM_SENTINEL) and np.all(cy["betas"][K:] == B.SYM_SENTINEL)
        assert np.all(cy["D"][kf:] == B.SYM_SENTINEL) and np.all(cy["f"][kf:] == B.SYM_SENTINEL)
        if c == 0:
            assert np.all(np.abs(V[:n, 0] - v0) <= 2.0 * np.spacing(np.abs(v0))), "start column"
            assert not cy["speculated"] and not cy["merge_on_device"] and not cy["kept_compared"]
        else:
            assert np.array_equal(V[:, kf], prev["V"][:, prev["K"]]), "v_kfirst is the previous cycle's v_K"
            assert cy["speculated"] == (cs["engine"] != "block1" and c >= 2)
            assert cy["kept_compared"] == (cs["engine"] != "block1")
            assert cy["kept_differ"] == 0, "the cycle changed its kept columns"
        # ---- R1 - R3 against the reference run from this cycle's own inputs
        Vr, alr, ber = L.reference_cycle(A, V, kf, K)
        qk, reuse_k = L.quantities(A, normA, cy, reuse)
        qr, _ = L.quantities(A, normA, dict(kfirst=kf, K=K, V=Vr, alphas=alr, betas=ber, D=cy["D"], f=cy["f"]), reuse_k)
        reuse = reuse_k
        print(O.ratio_lines(cs["id"], c, cy, qk, qr))
        # condition: the reference's own quantities are small, so no bound is vacuous
        assert all(qr[q] <= L.HOST_BOUND * np.sqrt(K) for q in L.QUANTITIES), qr
        assert qk["beta_min"] > 0.0
        for q in L.QUANTITIES:
            if not qk[q] <= L.bound(qr[q]):
                failures.append((c + 1, q, qk[q], qr[q], L.bound(qr[q])))
        if c > 0:
            res = L.span_residual(prev["V"][:n], prev["K"], V[:n, :kf])
            print(f"  span residual of the kept columns {res:.2e} (bound {L.bound(qr['r2']):.2e})")
            if not res <= L.bound(qr["r2"]):
                failures.append((c + 1, "span", res, qr["r2"], L.bound(qr["r2"])))
        prev = cy
    assert not failures, failures


@pytest.mark.parametrize("cs", O.STOP_CASES, ids=lambda c: c["id"])
def test_invariant_subspace_stops_the_cycle(cs):
    """the packed stop test restated on the operator form: F diag(9, 7, 5, 3, 2) F' with a zero diagonal E is an exact rank-5
    matrix, the Krylov space of the start vector has dimension 6.  The step that finds beta <= tol writes the stop flag and
    kstop and no basis column, later launches return at once (fop_body's and fop_owner_body's early-outs): from column kstop on
    the basis buffer holds what the zeroed workspace held, +0.0."""
    n = cs["n"]
    pcs = O.rank5_pieces(n)
    support, values, other, F, lam, normA = pcs
    A = O.Operator(n, support, values, F, lam)
    got = O.capture(dict(cs, cycles=3), pcs=pcs)
    assert len(got["cycles"]) == 1                                   # the driver ends the run on the invariant subspace
    cy = got["cycles"][0]
    K, V = cy["K"], cy["V"]
    assert cy["engine"] == cs["engine"] and cy["stop"] == 1 and K == 6 and cy["kfirst"] == 0
    assert cy["fop"] > 0 and cy["nchp"] == 1 and cy["ell_w"] == 1 and cy["owner"] == (cs["engine"] == "step")
    assert 0.0 <= cy["betas"][K - 1] <= L.TOL and np.all(cy["betas"][:K - 1] > 0.0)
    assert _positive_zero(V[:, K:]), "columns from kstop on"
    assert _positive_zero(V[n:, :K]), "padding rows"
    assert np.all(cy["alphas"][K:] == B.SYM_SENTINEL) and np.all(cy["betas"][K:] == B.SYM_SENTINEL)
    assert np.all(got["untouched"]["info"] == -1) and np.all(got["untouched"]["V"] == B.SYM_SENTINEL)
    head = dict(cy, K=K - 1)
    Vr, alr, ber = L.reference_cycle(A, V, 0, K - 1)
    qk, reuse = L.quantities(A, normA, head)
    qr, _ = L.quantities(A, normA, dict(head, V=Vr, alphas=alr, betas=ber), reuse)
    print(O.ratio_lines(cs["id"], 0, cy, qk, qr))
    assert all(qk[q] <= L.bound(qr[q]) for q in L.QUANTITIES), (qk, qr)
    Vl = V[:n, :K].astype(L.LD)
    last = L.times_a(A, V[:n, K - 1:K])[:, 0] - Vl[:, K - 2] * L.LD(cy["betas"][K - 2]) - Vl[:, K - 1] * L.LD(cy["alphas"][K - 1])
    assert float(np.abs(last).max()) <= L.TOL + L.bound(qr["r1_own"]) * normA


@pytest.mark.parametrize("cs", O.OWNER_CASES, ids=lambda c: c["id"])
def test_owner_form_is_the_records_form_bit_for_bit(cs, monkeypatch):
    """the same input with PROXSDP_HIP_FOP_OWNER = 0: every cycle's basis and coefficients are the same bits, the reported form
    differs"""
    own = O.capture(cs)
    monkeypatch.setenv("PROXSDP_HIP_FOP_OWNER", "0")
    rec = O.capture(cs)
    monkeypatch.delenv("PROXSDP_HIP_FOP_OWNER")
    assert len(own["cycles"]) == len(rec["cycles"]) == cs["cycles"]
    for x, y in zip(own["cycles"], rec["cycles"]):
        assert x["owner"] and not y["owner"] and x["fop"] == y["fop"] > 0
        for key in ("V", "alphas", "betas", "D", "f"):
            assert x[key].tobytes() == y[key].tobytes(), key
        assert all(x[k] == y[k] for k in ("kfirst", "K", "stop", "engine", "nchp", "ell_w", "speculated"))


def _relabelled(n, support, values, perm):
    """the same matrix with its rows and columns renumbered i -> perm[i]: another support list, another ELL / overflow layout"""
    i, j = O.unpacked_index(support)
    k = O.packed_index(perm[i], perm[j])
    order = np.argsort(k)
    return k[order], np.asarray(values)[order]


@pytest.mark.parametrize("cs", O.PROBE_CASES, ids=lambda c: c["id"])
def test_one_matvec_gives_e_v_row_by_row(cs):
    """ONE k_fop launch on the records form, outside any run: E v per row against the exact rational sum under the any-order
    bound nnz_i 2^-53 sum |terms| (an empty row exactly +0.0), the records of F' v per row block under the same bound, the row
    blocks' shares of v' E v.  The support list is ascending, so the only re-ordering of its values that leaves the matrix
    unchanged is a renumbering of rows and columns (with v renumbered too): the reversed numbering puts every row into another
    row block and slot and must satisfy the same bound."""
    n = cs["n"]
    support, values, other, F, lam, normA = O.cs_pieces(cs)
    rng = np.random.default_rng(11)
    v = rng.standard_normal(n)
    perm = np.arange(n)[::-1].copy()
    vp = np.zeros(n)
    vp[perm] = v
    s2, x2 = _relabelled(n, support, values, perm)
    F2 = np.zeros_like(F)
    F2[perm] = F
    for supp, vals, Fm, vec in ((support, values, F, v), (s2, x2, F2, vp)):
        A = O.Operator(n, supp, vals, Fm, lam)
        got = O.capture(cs, cycles=1, pcs=(supp, vals, np.full(len(supp), np.nan), Fm, lam, normA), probe_v=vec)
        pr = got["probe"]
        assert got["ell_w"] == 32 and got["overflow_rows"] == cs["overflow_rows"]
        bad = O.ev_rows_within_bound(A, vec, pr["ev"][:n])
        assert not bad, bad
        assert _positive_zero(pr["ev"][n:]), "padding rows of E v"
        u = Fraction(1, 2 ** 53)
        for g in range((n + 63) // 64):
            rows = range(64 * g, min(64 * g + 64, n))
            for c in range(cs["rp"]):
                terms = [Fraction(float(Fm[r, c])) * Fraction(float(vec[r])) for r in rows]
                err = abs(Fraction(float(pr["tpart"][g, c])) - sum(terms, Fraction(0)))
                assert err <= len(terms) * u * sum((abs(t) for t in terms), Fraction(0)), ("record", g, c)
            terms = [Fraction(float(pr["ev"][r])) * Fraction(float(vec[r])) for r in rows]
            err = abs(Fraction(float(pr["apart"][g])) - sum(terms, Fraction(0)))
            assert err <= len(terms) * u * sum((abs(t) for t in terms), Fraction(0)), ("share of v'Ev", g)


@pytest.mark.parametrize("cs", O.WARM_CASES, ids=lambda c: c["id"])
def test_warm_start_column(cs):
    """lanczos_warm_start = 1: k_lz_warm_sum writes v_i = sum_c F_ic + 1e-3 resid_i (Krylov branch: no weights), k_lz_warm_scale
    divides by the square root of the sum of squares and clears the control block.  Column 0 of cycle 1 against that in long
    double: per entry the any-order bound of the rp + 1 terms and one rounding for the scale (and the library's own
    normalisation of the start vector, 2 ulp of the 1e-3 term), norm 1 to 4 x 2^-52, padding rows +0.0; the cycle runs to K."""
    n, rp = cs["n"], cs["rp"]
    support, values, other, F, lam, normA = O.cs_pieces(cs)
    got = O.capture(cs, cycles=1, lanczos_warm_start=1)
    cy = got["cycles"][0]
    assert cy["engine"] == cs["engine"] and cy["stop"] == 0 and cy["K"] == cs["kd"] and cy["kfirst"] == 0 and cy["fop"] == cs["kd"]
    col = cy["V"][:, 0]
    r0 = L.start(n)
    Fl, rl = F.astype(L.LD), L.LD(1e-3) * r0.astype(L.LD)
    v = Fl.sum(axis=1) + rl
    mag = np.abs(Fl).sum(axis=1) + np.abs(rl)
    s = np.sqrt((v * v).sum())
    want = v / s
    u = L.LD(2.0) ** -53
    bnd = ((rp + 1) * u * mag + 4 * u * np.abs(rl)) / s + u * np.abs(want)
    err = np.abs(col[:n].astype(L.LD) - want)
    print(f"warm start {cs['id']}: largest error / bound {float((err / bnd).max()):.3f}")
    assert np.all(err <= bnd), float((err / bnd).max())
    assert abs(float(np.sqrt((col.astype(L.LD) ** 2).sum())) - 1.0) <= 4 * L.EPS
    assert _positive_zero(col[n:]), "padding rows"
    # the cycle that followed is a Lanczos decomposition from that column, by the rule of the first test
    A, _ = O.operator(cs)
    Vr, alr, ber = L.reference_cycle(A, cy["V"], 0, cy["K"])
    qk, reuse = L.quantities(A, normA, cy)
    qr, _ = L.quantities(A, normA, dict(cy, V=Vr, alphas=alr, betas=ber), reuse)
    print(O.ratio_lines(cs["id"] + "-warm", 0, cy, qk, qr))
    assert qk["beta_min"] > 0.0 and all(qk[q] <= L.bound(qr[q]) for q in L.QUANTITIES), (qk, qr)
