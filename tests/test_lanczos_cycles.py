"""Every cycle of the production Lanczos driver against exact checks (proxsdp_hip_lanczos_cycles: Solver::lanczos with its
per-cycle observer installed, ended by the driver itself after max_cycles).

  step kernels    k_symv_packed, k_symv_finish<NCH>, k_lz_orth<NCH, 0>, k_lz_finish<NCH>      NCH = 1 .. 4, n > 4096
  block1          k_lz_block1 with its deferred restart rotation
  wide kernels    k_lzw_dots / _reduce / _update / _close, k_lzw_rotate

For each captured cycle, in long double (lanczos_cycle_cases.quantities): R1 the Krylov-Schur relation A V = V Tbar (all
columns, and the cycle's own), R2 orthonormality of all K + 1 columns (and of the cycle's new columns against all), R3
alpha_k = v_k' A v_k and beta_k = v_{k+1}' A v_k, and beta_k > 0.  The bound of a quantity is MARGIN = 8 times what the plain
fp64 reference (two measured Gram-Schmidt passes, lanczos_cycle_cases.reference_cycle) gives from the SAME cycle's inputs,
with the floor 8 x 2^-52.  Exact hand-over checks:
padding rows, the start column, v_kfirst = the previous cycle's v_K bit for bit, the kept columns inside the previous span.

Out of scope: lanczos_eager and lanczos_batch: bit-for-bit tests tie the batched path to the per-block one.  The operator form
(k_fop*, k_lz_orth<., 1 | 2>, k_lz_block1<., true>) has a hook of its own, held to the same rule: test_operator_cycles.py.
The positive-part run (full_eig! served by this engine: another Krylov dimension, acceptance rule and start) and its certificate
(k_lz_measure, the step kernels from kfirst = npos) have theirs, held to the same rule too: test_positive_part.py.

The kept columns: after a restart on the step or wide engine the entry repeats the restart rotation (Solver::rotate_launch on
the previous basis and the coefficients still on the device) into a buffer of its own and counts the entries of the columns
0 .. kfirst whose bits differ from the cycle's: a cycle does not touch its kept part.  (The reference cycle starts from the
snapshot's kept columns, so without this a cycle that spoilt them would spoil its own yardstick too.)  k_lz_block1 rotates in
its prologue: the span check applies there."""
import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import lanczos_cycle_cases as L

pytestmark = pytest.mark.gpu


def _options(opts):
    o = B.default_options()
    for k, v in opts.items():
        B.set_option(o, k, v)
    return o


def _capture(cs, packed, cycles):
    return B.lanczos_cycles(packed, cs["n"], cs["nev"], cycles, options=_options(cs["opts"]))


def _positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


@pytest.mark.parametrize("cs", L.CASES, ids=[c["id"] for c in L.CASES])
def test_every_cycle_is_a_krylov_schur_decomposition(cs):
    n, kd = cs["n"], cs["kd"]
    A, packed, normA = L.matrix(n, cs["nev"])
    got = _capture(cs, packed, cs["cycles"])
    cyc = got["cycles"]
    assert got["krylovdim"] == kd and got["npad"] == 64 * ((n + 63) // 64)
    # condition: the restarted cycles were captured
    assert len(cyc) == cs["cycles"], (len(cyc), cs["cycles"])
    assert got["untouched"]["info"].size == 0
    v0 = L.start(n)
    lines, failures, prev, reuse = [], [], None, None
    for c, cy in enumerate(cyc):
        K, kf, V = cy["K"], cy["kfirst"], cy["V"]
        assert cy["engine"] == cs["engine"] and cy["stop"] == 0 and K == kd
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
        lines.append(L.ratio_lines(cs["id"], c, cy, qk, qr))
        print(lines[-1])
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
    for flag in cs["flags"]:
        assert any(cy[flag] for cy in cyc), flag
    if "split" in cs["flags"]:
        assert all(cy["split"] and cy["split_ready"] for cy in cyc)
    if "merge_on_device" in cs["flags"]:
        assert all(cy["merge_on_device"] for cy in cyc[1:])


@pytest.mark.parametrize("cs", L.STOP_CASES, ids=[c["id"] for c in L.STOP_CASES])
def test_invariant_subspace_stops_the_cycle(cs):
    """an exact rank-5 matrix: the Krylov space of the start vector has dimension 6.  The step that finds beta <= tol writes the
    stop flag and kstop and no basis column (k_lz_finish / k_symv_finish return before the store of v_{k+1}, k_lz_block1's
    epilogue stores the columns 0 .. kstop - 1), later launches return at once: from column kstop on the basis buffer holds
    what the zeroed workspace held, +0.0."""
    n, kd = cs["n"], cs["kd"]
    A, packed, normA = L.rank5_matrix(n)
    got = _capture(cs, packed, 3)
    assert len(got["cycles"]) == 1                                   # the driver ends the run on the invariant subspace
    cy = got["cycles"][0]
    K, V = cy["K"], cy["V"]
    assert cy["engine"] == cs["engine"] and cy["stop"] == 1 and K == 6 and cy["kfirst"] == 0
    assert 0.0 <= cy["betas"][K - 1] <= L.TOL and np.all(cy["betas"][:K - 1] > 0.0)
    assert _positive_zero(V[:, K:]), "columns from kstop on"
    assert _positive_zero(V[n:, :K]), "padding rows"
    assert np.all(cy["alphas"][K:] == B.SYM_SENTINEL) and np.all(cy["betas"][K:] == B.SYM_SENTINEL)
    assert np.all(got["untouched"]["info"] == -1) and np.all(got["untouched"]["V"] == B.SYM_SENTINEL)
    # the K columns that were written: steps 0 .. K - 2 are a Lanczos decomposition with v_{K-1} as its residual column, held
    # to the rule of the test above; the last step closes it without one (beta_{K-1} <= tol)
    head = dict(cy, K=K - 1)
    Vr, alr, ber = L.reference_cycle(A, V, 0, K - 1)
    qk, reuse = L.quantities(A, normA, head)
    qr, _ = L.quantities(A, normA, dict(head, V=Vr, alphas=alr, betas=ber), reuse)
    print(L.ratio_lines(cs["id"], 0, cy, qk, qr))
    assert all(qk[q] <= L.bound(qr[q]) for q in L.QUANTITIES), (qk, qr)
    Vl = V[:n, :K].astype(L.LD)
    last = L.times_a(A, V[:n, K - 1:K])[:, 0] - Vl[:, K - 2] * L.LD(cy["betas"][K - 2]) - Vl[:, K - 1] * L.LD(cy["alphas"][K - 1])
    assert float(np.abs(last).max()) <= L.TOL + L.bound(qr["r1_own"]) * normA


def test_two_runs_give_bit_equal_snapshots():
    cs = next(c for c in L.CASES if c["n"] == 257 and c["engine"] == "step" and "split" in c["flags"])
    _, packed, _ = L.matrix(cs["n"], cs["nev"])
    a, b = _capture(cs, packed, cs["cycles"]), _capture(cs, packed, cs["cycles"])
    assert len(a["cycles"]) == len(b["cycles"]) == cs["cycles"]
    for x, y in zip(a["cycles"], b["cycles"]):
        for key in ("V", "alphas", "betas", "D", "f"):
            assert x[key].tobytes() == y[key].tobytes(), key
        assert all(x[k] == y[k] for k in ("kfirst", "K", "stop", "engine", "split", "speculated", "merge_on_device"))
