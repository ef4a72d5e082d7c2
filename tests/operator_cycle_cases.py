"""Cases, operator and references of the per-cycle tests of the Lanczos engine on the OPERATOR FORM (test_operator_cycles.py on
the GPU, test_operator_cycles_host.py on the CPU).  The checks, the plain fp64 reference cycle, the restart, MARGIN, FLOOR and
HOST_BOUND are lanczos_cycle_cases': they take the `Operator` below where they take a dense matrix.

The matrix is known by its pieces only,  A = F diag(lam) F' + E:  F (n x rp, orthonormal columns) and lam the previous
projection's factors, E a sparse symmetric matrix given as the solver holds it -- a support list of ascending packed indices
k = i + j (j + 1) / 2 (i <= j, column-major upper triangle) with one value each in svec units: the diagonal value as it is,
an off-diagonal value divided by sqrt(2) and mirrored.  That definition is all this file takes from the library: the ELL and
overflow layout the kernels read is built by the library's own set-up code and never restated here."""
import functools
import math
from fractions import Fraction

import numpy as np

import lanczos_cycle_cases as L

LD = L.LD
SEED = 77100
LDS_CAP_DOUBLES = 160 * 1024 // 8                  # gfx950: 160 KiB of LDS per workgroup, what k_lz_block1 is granted


# ------------------------------------------------------------------------------------------------ packed indices
def packed_index(i, j):
    i, j = np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)
    return i + j * (j + 1) // 2


def unpacked_index(k):
    k = np.asarray(k, dtype=np.int64)
    j = ((np.sqrt(8.0 * k + 1.0) - 1.0) / 2.0).astype(np.int64)
    j = np.where((j + 1) * (j + 2) // 2 <= k, j + 1, j)
    j = np.where(j * (j + 1) // 2 > k, j - 1, j)
    i = k - j * (j + 1) // 2
    assert np.all((0 <= i) & (i <= j))
    return i, j


# ------------------------------------------------------------------------------------------------ the operator
class Operator:
    """A = F diag(lam) F' + E from the pieces.  `A @ v`: plain fp64 (the yardstick's mat-vec); times_ld(V): every product in
    long double (the truth).  variant: a deliberately wrong operator (the host test shows that the checks tell each apart) --
    "drop_overflow": the last entry of the widest row is left out (its mirror image stays); "no_sqrt2": one off-diagonal entry
    keeps its svec value; "no_mirror": one off-diagonal entry has no mirror image; "lam64": the factor column 64 is left out;
    "other_half": E takes `other`, the values of the other half of the support-value array."""

    def __init__(self, n, support, values, F, lam, variant=None, other=None):
        self.n, self.shape = n, (n, n)
        self.support = np.asarray(support, dtype=np.int64)
        self.values = np.asarray(values, dtype=np.float64)
        if variant == "other_half":
            self.values = np.asarray(other, dtype=np.float64)
        self.F = np.asarray(F, dtype=np.float64).reshape(n, -1)
        self.lam = np.asarray(lam, dtype=np.float64).copy()
        assert np.all(np.diff(self.support) > 0) and len(self.values) == len(self.support) and len(self.lam) == self.F.shape[1]
        if variant == "lam64":
            self.lam[64] = 0.0
        i, j = unpacked_index(self.support) if len(self.support) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        off = i != j
        self.rows = np.concatenate([i, j[off]])
        self.cols = np.concatenate([j, i[off]])
        unit = np.concatenate([np.zeros(len(i), bool) | ~off, np.zeros(int(off.sum()), bool)])    # True: the value as it is
        val = np.concatenate([self.values, self.values[off]])
        keep = np.ones(len(val), bool)
        offs = np.flatnonzero(off)
        if variant == "no_sqrt2":
            unit[offs[len(offs) // 2]] = True
        elif variant == "no_mirror":
            keep[len(i) + len(offs) // 2] = False
        elif variant == "drop_overflow":
            cnt = np.bincount(self.rows, minlength=n)
            hub = int(np.argmax(cnt))
            assert cnt[hub] > 32
            keep[np.flatnonzero(self.rows == hub)[-1]] = False
        elif variant not in (None, "lam64", "other_half"):
            raise ValueError(variant)
        self.rows, self.cols, unit, val = self.rows[keep], self.cols[keep], unit[keep], val[keep]
        self.e64 = np.where(unit, val, val / math.sqrt(2.0))
        self.eld = np.where(unit, val.astype(LD), val.astype(LD) / np.sqrt(LD(2)))
        self.Fld, self.lamld = self.F.astype(LD), self.lam.astype(LD)

    def __matmul__(self, v):
        v = np.asarray(v, dtype=np.float64)
        assert v.shape == (self.n,)
        return self.F @ (self.lam * (self.F.T @ v)) + np.bincount(self.rows, weights=self.e64 * v[self.cols], minlength=self.n)

    def times_ld(self, V):
        Vl = np.asarray(V)[:self.n].astype(LD)
        out = self.Fld @ (self.lamld[:, None] * (self.Fld.T @ Vl))
        np.add.at(out, self.rows, self.eld[:, None] * Vl[self.cols])
        return out

    def dense_e(self):
        E = np.zeros((self.n, self.n))
        np.add.at(E, (self.rows, self.cols), self.e64)
        return E

    def dense(self):
        return (self.F * self.lam) @ self.F.T + self.dense_e()

    def row_counts(self):
        return np.bincount(self.rows, minlength=self.n)


# ------------------------------------------------------------------------------------------------ row patterns
def _pairs_to_support(pairs):
    p = np.array(sorted(set((min(a, b), max(a, b)) for a, b in pairs)), dtype=np.int64).reshape(-1, 2)
    return np.sort(packed_index(p[:, 0], p[:, 1]))


def pattern_diag(n, rng):
    """the diagonal alone (ell_w = 1: Max-Cut's pattern)"""
    return _pairs_to_support([(i, i) for i in range(n)])


def pattern_sparse(n, rng):
    """the diagonal and two random off-diagonal entries a row (so about five entries a row after mirroring)"""
    pairs = [(i, i) for i in range(n)]
    for i in range(n):
        for j in rng.choice(n, 2, replace=False):
            if j != i:
                pairs.append((i, int(j)))
    return _pairs_to_support(pairs)


ROUNDS = {3: 1, 10: 15, 64: 16, 77: 17, 128: 31, 129: 32}        # row: entries (n = 130; rows 128, 129: the partial last block)
ROUNDS_EMPTY = 5


def pattern_rounds(n, rng):
    """n = 130: rows of exactly 1, 15, 16, 17, 31 and 32 entries and one empty row -- the prefetched first round of 16 entries
    a row (four a wave) full, short by one and over by one, the second round the same.  The counted rows have no diagonal entry
    and meet only filler rows, which have one"""
    assert n == 130
    fill = [r for r in range(n) if r not in ROUNDS and r != ROUNDS_EMPTY]
    pairs = [(r, r) for r in fill]
    for r, cnt in ROUNDS.items():
        pairs += [(r, int(c)) for c in rng.choice(fill, cnt, replace=False)]
    return _pairs_to_support(pairs)


OVER_HUB, OVER_WIDE, OVER_33 = 70, 100, 5                       # hub and a 40-entry row in the same 64-row block; a 33-entry row


def pattern_overflow(n, rng):
    """n = 330: row 5 has 33 entries (one overflow entry); row 70 (the hub) 300 -- 268 overflow entries, so the workgroup's
    loop of 256 threads over them runs twice; row 100, in the hub's row block, 40; row 329, the last row, in the partial last
    block, 40.  Every other row stays below the ELL width of 32"""
    assert n == 330
    pairs = [(i, i) for i in range(n)]
    skip = set(range(200, 230))
    pairs += [(OVER_HUB, c) for c in range(n) if c != OVER_HUB and c not in skip]              # 299 + the diagonal = 300
    fill = [r for r in range(n) if r not in (OVER_HUB, OVER_WIDE, OVER_33, n - 1) and r not in skip]
    for r, extra in ((OVER_WIDE, 38), (n - 1, 38), (OVER_33, 31)):                             # + the hub + the diagonal
        pairs += [(r, int(c)) for c in rng.choice(fill, extra, replace=False)]
    return _pairs_to_support(pairs)


def pattern_wide32(n, rng):
    """the sparse pattern and one row of exactly 32 entries (ell_w = 32, no overflow)"""
    pairs = [(i, i) for i in range(n)] + [(i, (i + 1) % n) for i in range(0, n, 2)]
    r = n // 2
    have = {r, (r + 1) % n, (r - 1) % n}
    rest = [c for c in range(n) if c not in have]
    cnt = 1 + (1 if r % 2 == 0 else 0) + (1 if (r - 1) % 2 == 0 else 0)
    pairs += [(r, int(c)) for c in rng.choice(rest[::3], 32 - cnt, replace=False)]
    return _pairs_to_support(pairs)


PATTERNS = dict(diag=pattern_diag, sparse=pattern_sparse, rounds=pattern_rounds, overflow=pattern_overflow, wide32=pattern_wide32)


# ------------------------------------------------------------------------------------------------ the matrices
@functools.lru_cache(maxsize=None)
def pieces(n, nev, rp, pattern, no_factors=False):
    """(support, values, other, F, lam, normA) of a case: F orthonormal, lam = linspace(12, 10, nev + 4) cut to rp or padded with
    smaller positive values, E random on the pattern with |E|_2 <= 1 (n <= 400: the exact norm; above: the largest absolute row
    sum).  no_factors: A = E with nev + 4 diagonal entries raised to linspace(12, 10, nev + 4).  other: the values of the other
    half of the support-value array (what the form must not read).  normA: exact (eigvalsh) for n <= 400, else max(lam) + the
    largest absolute row sum of E -- an upper bound, which loosens the reference and the kernel by the same factor."""
    rng = np.random.default_rng(SEED + 7919 * n + 101 * nev + 13 * rp + (1 if no_factors else 0))
    support = PATTERNS[pattern](n, rng)
    i, j = unpacked_index(support)
    values = rng.standard_normal(len(support)) * np.where(i == j, 1.0, math.sqrt(2.0))
    top = np.linspace(12.0, 10.0, nev + 4)
    if rp > 0:
        F, _ = np.linalg.qr(rng.standard_normal((n, rp)))
        lam = top[:rp] if rp <= nev + 4 else np.concatenate([top, rng.uniform(1.0, 8.0, rp - nev - 4)])
    else:
        F, lam = np.zeros((n, 0)), np.zeros(0)
    E = Operator(n, support, values, np.zeros((n, 0)), np.zeros(0))
    scale = np.abs(np.linalg.eigvalsh(E.dense_e())).max() if n <= 400 else np.bincount(E.rows, weights=np.abs(E.e64), minlength=n).max()
    values = values / scale
    if no_factors:
        diag = np.flatnonzero(i == j)
        assert len(diag) >= nev + 4
        values[rng.choice(diag, nev + 4, replace=False)] = top
    other = rng.standard_normal(len(support)) / 4.0
    A = Operator(n, support, values, F, lam)
    if n <= 400:
        normA = float(np.abs(np.linalg.eigvalsh(A.dense())).max())
    else:
        normA = float((lam.max() if rp > 0 else 0.0) + np.bincount(A.rows, weights=np.abs(A.e64), minlength=n).max())
    for a in (support, values, other, F, lam):
        a.setflags(write=False)
    return support, values, other, F, lam, normA


@functools.lru_cache(maxsize=None)
def rank5_pieces(n):
    """the packed stop cases restated: F holds lanczos_cycle_cases.rank5_matrix's five disjoint +-1/4 vectors, lam = (9, 7, 5, 3, 2),
    the support is the diagonal with zero values -- an exact rank-5 matrix, every product a small integer over 16"""
    rng = np.random.default_rng(L.SEED + n)
    perm = rng.permutation(n)
    F = np.zeros((n, 5))
    for q in range(5):
        F[perm[q * 16:(q + 1) * 16], q] = rng.choice([-1.0, 1.0], 16) / 4.0
    lam = np.array([9.0, 7.0, 5.0, 3.0, 2.0])
    assert np.array_equal((F * lam) @ F.T, L.rank5_matrix(n)[0])
    support = pattern_diag(n, None)
    return support, np.zeros(n), np.zeros(n), F, lam, 9.0


def operator(cs, variant=None):
    support, values, other, F, lam, normA = cs_pieces(cs)
    return Operator(cs["n"], support, values, F, lam, variant=variant, other=other), normA


def cs_pieces(cs):
    return pieces(cs["n"], cs["nev"], cs["rp"], cs["pattern"], cs["no_factors"])


# ------------------------------------------------------------------------------------------------ the cases
def owner_rule(n, rp, engine):
    """the form lz_plan documents: column owners on the step kernels where nt <= 64 row blocks hold 1 <= rp <= 2 nt columns"""
    nt = (n + 63) // 64
    return engine == "step" and nt <= 64 and 0 < rp <= 2 * nt


def case(n, nev, kd, rp, pattern, engine, tag, cycles=3, ell_w=None, overflow_rows=0, ell_in_lds=None, no_factors=False,
         f_first=0, owner=None, **opts):
    o = dict(eigsolver_min_lanczos=kd)
    o.update(opts)
    assert kd == max(2 * nev + 1, kd) and (rp == 0 or not no_factors)
    return dict(n=n, nev=nev, kd=kd, rp=rp, pattern=pattern, engine=engine, cycles=cycles, ell_w=ell_w, overflow_rows=overflow_rows,
                ell_in_lds=ell_in_lds, no_factors=no_factors, f_first=f_first, opts=o,
                owner=owner_rule(n, rp, engine) if owner is None else owner, nchp=1 if rp <= 64 else 2,
                id=f"n{n}-rp{rp}{'-nofactors' if no_factors else ''}-nev{nev}-K{kd}-{tag}")


def expect_ell_in_lds(cs, A):
    """what k_lz_block1 must report for the case: E resident in LDS where b1_lds_plan with the case's ELL width fits the LDS of
    a workgroup (launch_block1's rule), read through L2 otherwise; None on the step kernels"""
    from proxsdp_jl_amd import binding as B
    if cs["engine"] != "block1":
        return None
    ell_w = min(max(int(A.row_counts().max()), 1), 32)
    want = B.block1_lds_doubles((cs["n"] + 63) // 64, True, 0, ell_w) <= LDS_CAP_DOUBLES
    assert cs["ell_in_lds"] in (None, want)
    return want


def l2_side():
    """the smallest side at which the one-workgroup kernel keeps a 32-wide E out of LDS: the smallest nt <= 8 whose plan with
    ell_w = 32 resident exceeds the LDS of a workgroup while the plan without E fits (block1_plan's own condition)"""
    from proxsdp_jl_amd import binding as B
    for nt in range(1, 9):
        if B.block1_lds_doubles(nt, True, 0, 0) <= LDS_CAP_DOUBLES < B.block1_lds_doubles(nt, True, 0, 32):
            return 64 * (nt - 1) + 1
    return None


STEP, B1 = dict(lanczos_cycle_kernel=0), dict(lanczos_cycle_kernel=2)
# n, nev, krylovdim, factor rank, row pattern, the engine lz_plan must choose, tag; what the run must report.  nev > rp in the
# small cases: the wanted pairs beyond the factors' lie in the bulk of E, so the run restarts as often as it is asked to.
# cycles: 3, or 2 where the fp64 reference run has converged at the end of its second cycle (test_operator_cycles_host.py).
CASES = [
    # one row block, diagonal-only support / a last row block of one row
    case(64, 5, 12, 3, "diag", "step", "step", ell_w=1, **STEP),
    case(64, 5, 12, 3, "diag", "block1", "block1", ell_w=1),
    case(65, 8, 17, 6, "sparse", "step", "step", **STEP),
    case(65, 8, 17, 6, "sparse", "block1", "block1"),
    # the one-workgroup kernel's factor limit: rank 16 runs there with E in LDS, rank 17 falls to the step kernels under auto
    case(129, 14, 30, 16, "sparse", "block1", "auto", cycles=2, ell_in_lds=True),
    case(129, 14, 30, 17, "sparse", "step", "auto"),
    case(129, 14, 30, 16, "sparse", "step", "step", cycles=2, **STEP),
    # ELL rounds: 1, 15, 16, 17, 31, 32 entries a row and an empty row
    case(130, 10, 24, 6, "rounds", "step", "step", ell_w=32, **STEP),
    case(130, 10, 24, 6, "rounds", "block1", "block1", ell_w=32, ell_in_lds=False),   # (three row blocks of 32 entries: through L2)
    # overflow rows; the one-workgroup kernel refuses them even when asked for
    case(330, 10, 24, 6, "overflow", "step", "b1refused", ell_w=32, overflow_rows=4, lanczos_operator=1, lanczos_cycle_kernel=2),
    # the factor rank across one 64-column chunk, records form (NCH = 2)
    case(257, 34, 70, 63, "sparse", "step", "step"),
    case(257, 34, 70, 64, "sparse", "step", "step"),
    case(257, 34, 70, 65, "sparse", "step", "step"),
    case(257, 34, 70, 127, "sparse", "step", "step"),
    # owner form: one column an owner, two, 2 nt; one more is the records form; NCHP = 2 on owners
    case(400, 10, 24, 7, "sparse", "step", "step"),
    case(400, 10, 24, 8, "sparse", "step", "step"),
    case(400, 10, 24, 14, "sparse", "step", "step"),
    case(400, 10, 24, 15, "sparse", "step", "step"),
    case(2100, 10, 24, 66, "sparse", "step", "step"),
    # nt = 65, pld = 128: every "n > 4096" loop
    case(4097, 3, 8, 3, "sparse", "step", "step"),
    case(4097, 3, 8, 65, "sparse", "step", "step"),
    case(4097, 3, 8, 0, "sparse", "step", "step", no_factors=True),
    # no factors: the values at esv + ns
    case(129, 8, 20, 0, "sparse", "block1", "auto", no_factors=True),
    case(300, 8, 20, 0, "sparse", "step", "step", no_factors=True),
    # restarts with keep > 64 (NCH = 3 with NCHP = 2)
    case(300, 64, 130, 70, "sparse", "step", "step", cycles=2),
    # dsaupd's rule, the factors not at column 0 of their buffer (as its ascending order leaves them)
    case(257, 34, 70, 34, "sparse", "step", "arpack", cycles=2, f_first=3, eigsolver=1),
]
STOP_CASES = [dict(n=130, nev=8, kd=30, rp=5, engine=e, opts=dict(eigsolver_min_lanczos=30, lanczos_cycle_kernel=k), id=f"rank5-{e}")
              for e, k in (("step", 0), ("block1", 2))]
WARM_CASES = [c for c in CASES if (c["n"], c["rp"], c["id"].rsplit("-", 1)[1]) in ((129, 16, "auto"), (400, 14, "step"))]
OWNER_CASES = [c for c in CASES if c["owner"]]
PROBE_CASES = [c for c in CASES if c["pattern"] in ("rounds", "overflow") and c["engine"] == "step"]


def l2_case():
    """block1 with E read through L2 (ell_in_lds = 0), or None where no legal shape reaches it"""
    n = l2_side()
    if n is None:
        return None
    return case(n, 10, 24, 6, "wide32", "block1", "block1-l2", ell_w=32, ell_in_lds=False, **B1)


def reference_cycles(cs):
    """the fp64 reference run of a case: (cycles, converged before the last of them)"""
    A, _ = operator(cs)
    arpack = cs["opts"].get("eigsolver", 2) == 1
    return L.reference_run(A, L.start(cs["n"]), cs["nev"], cs["kd"], cs["cycles"], tol=1e-10 if arpack else L.TOL, arpack=arpack)


# ------------------------------------------------------------------------------------------------ E v and F'v, exactly
def ev_rows_within_bound(A, v, got):
    """every row of E v on its own, by the bound tests/test_gpu_parity.py _spmv_rows_within_bound states: |got_i - sum_j e_ij v_j|
    <= nnz_i 2^-53 sum_j |e_ij v_j| (one rounding per product and per addition, in any order), the sum in rational arithmetic;
    an empty row is exactly +0.0.  e_ij is the fp64 matrix entry: the diagonal value, or off the diagonal the ONE fp64 product
    of the svec value and the fp64 nearest 1 / sqrt(2).  Returns the failing rows."""
    inv = 0.70710678118654752440
    i, j = unpacked_index(A.support)
    terms = [[] for _ in range(A.n)]
    for a, b, val in zip(i, j, A.values):
        if a == b:
            terms[a].append(Fraction(float(val)) * Fraction(float(v[a])))
        else:
            e = Fraction(float(val) * inv)
            terms[a].append(e * Fraction(float(v[b])))
            terms[b].append(e * Fraction(float(v[a])))
    bad = []
    for r in range(A.n):
        if not terms[r]:
            if not (got[r] == 0.0 and not np.signbit(got[r])):
                bad.append((r, 0, float(got[r]), 0.0))
            continue
        exact, mag = sum(terms[r], Fraction(0)), sum((abs(t) for t in terms[r]), Fraction(0))
        err = abs(Fraction(float(got[r])) - exact)
        if err > len(terms[r]) * Fraction(1, 2 ** 53) * mag:
            bad.append((r, len(terms[r]), float(got[r]), float(exact)))
    return bad


# ------------------------------------------------------------------------------------------------ running a case (GPU)
def capture(cs, cycles=None, pcs=None, **kw):
    """the case through proxsdp_hip_operator_cycles (binding.operator_cycles); kw: options on top of the case's, or the
    binding's own arguments (probe_v, resid)"""
    from proxsdp_jl_amd import binding as B
    support, values, other, F, lam, _ = pcs if pcs is not None else cs_pieces(cs)
    o = B.default_options()
    args = {k: kw.pop(k) for k in ("probe_v", "resid") if k in kw}
    for k, v in dict(cs["opts"], **kw).items():
        B.set_option(o, k, v)
    return B.operator_cycles(cs["n"], support, values, F, lam, cs["nev"], cs["cycles"] if cycles is None else cycles, options=o,
                             no_factors=cs.get("no_factors", False), f_first=cs.get("f_first", 0), other_half=other, **args)


def ratio_lines(cid, c, cyc, qk, qr):
    """lanczos_cycle_cases.ratio_lines with the operator form's paths: the form of F'v, the chunks of factor columns, E's width"""
    form = "block1" + ("+lds" if cyc["ell_in_lds"] else "+l2") if cyc["engine"] == "block1" else ("owner" if cyc["owner"] else "records")
    paths = f"{form}, NCHP {cyc['nchp']}, ell_w {cyc['ell_w']}" + (f", {cyc['overflow_rows']} overflow rows" if cyc["overflow_rows"] else "")
    fields = L.ratio_lines(cid, c, cyc, qk, qr).split(" | ")
    fields[4] += f" ({paths})"
    return " | ".join(fields)
