"""Inputs and references for the one-launch small-block projections (k_small_psd_project, k_small_sign_project) as the solver
launches them; shared by test_small_blocks_host.py (CPU) and test_small_blocks.py (GPU, through proxsdp_hip_project_cones).

A case is X = Q diag(w) Q' with Q a product of Householder reflectors formed in np.longdouble and a chosen spectrum w.  The
input is X rounded to float64, the expected projection is Q diag(max(w, 0)) Q' evaluated in longdouble.  The projection onto the
PSD cone is non-expansive in the Frobenius norm, so the reference's error against the float64 input is at most
|X64 - Xld|_F + 2 |Q'Q - I|_F max|w| (the nearest orthogonal matrix lies within |Q'Q - I| / 2 of Q; replacing Q by it moves X
and its projection by at most twice that times max|w| each ... the second term is ~1e-18 max|w| in longdouble).  No LAPACK.

restated_jacobi() is a plain NumPy restatement of the kernel's round-robin cyclic Jacobi (same pair schedule, same rotation
formulas).  It takes NO part in the value checks; it only gives s_ref, the sweep count the stopping test should reach.
"""
import functools
import zlib

import numpy as np

LD = np.longdouble
TOL_PSD = 1e-7                                   # options.tol_psd default: current_rank counts eigenvalues above it
SIDES = (1, 2, 64, 3, 1, 17, 2, 33, 16, 48, 5, 65, 31, 2)
SOC_LEN, N_FREE, N_PAD = 5, 7, 70000
LAYOUTS = {"mixed": N_FREE, "padded": N_FREE + N_PAD}
SPECTRA = ("indefinite", "posdef", "negdef", "decades", "repeated", "diagonal", "zero", "aI_bee", "tiny", "huge")
DEALS = len(SPECTRA)                             # deal d gives the j-th block of side >= 2 spectrum (j + d) mod 10
TINY, HUGE = 2.0 ** -600, 2.0 ** 520
SQRT2 = np.sqrt(LD(2))


def packed_len(n):
    return n * (n + 1) // 2


def svec(X):
    """packed upper triangle, column by column, off-diagonals times sqrt 2 (the solver's internal scaling), float64"""
    n = X.shape[0]
    out = np.empty(packed_len(n))
    s2 = np.sqrt(2.0)
    t = 0
    for j in range(n):
        out[t:t + j] = X[:j, j] * s2
        out[t + j] = X[j, j]
        t += j + 1
    return out


def smat_ld(x, n):
    """inverse of svec, evaluated in longdouble (the comparison adds no float64 rounding of its own)"""
    X = np.zeros((n, n), dtype=LD)
    x = np.asarray(x).astype(LD)
    t = 0
    for j in range(n):
        X[:j, j] = x[t:t + j] / SQRT2
        X[j, :j] = X[:j, j]
        X[j, j] = x[t + j]
        t += j + 1
    return X


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def householder_q(n, rng):
    """product of n Householder reflectors, formed in longdouble"""
    Q = np.eye(n, dtype=LD)
    for _ in range(n):
        v = rng.standard_normal(n).astype(LD)
        v /= np.sqrt((v * v).sum())
        Q = Q - LD(2) * np.outer(Q @ v, v)
    return Q


def spectrum(kind, n, rng):
    if kind in ("indefinite", "diagonal"):
        w = rng.standard_normal(n)
        w[np.abs(w) < 1e-3] = 0.5                # (keeps every eigenvalue away from 0 and tol_psd)
        w[0], w[-1] = abs(w[0]) + 0.1, -abs(w[-1]) - 0.1
        return w
    if kind == "posdef":
        return rng.uniform(0.05, 3.0, n)
    if kind == "negdef":
        return -rng.uniform(0.05, 3.0, n)
    if kind in ("decades", "tiny", "huge"):
        npos = n // 2
        ep, en = rng.uniform(-6, 2, npos), rng.uniform(-6, 2, n - npos)
        ep[0], en[-1] = 2.0, -6.0                # the full eight decades at every side
        return np.concatenate([10.0 ** ep, -(10.0 ** en)])
    if kind == "repeated":
        k = n // 3
        return np.concatenate([np.full(k, 2.0), np.full(k, -0.5), np.zeros(n - 2 * k)])
    if kind == "zero":
        return np.zeros(n)
    raise KeyError(kind)


class Case:
    """X64: the float64 input; ref: the expected projection (longdouble); w: the spectrum (longdouble); scale = max |w|;
    ref_err: bound on |ref - projection of X64| (Frobenius, hence entrywise); s_ref: see restated_jacobi"""

    def __init__(self, kind, n, X64, ref, w, ref_err, base=None):
        self.kind, self.n, self.X64, self.ref, self.w, self.ref_err = kind, n, X64, ref, w, ref_err
        self.scale = float(np.abs(w).max()) if n else 0.0
        self.base = base                         # tiny / huge: the unscaled eight-decade case
        self.x = svec(X64)
        # thresholds: rank counts are unambiguous
        nz = w[w != 0]
        assert not np.any(np.abs(nz) <= 1e-9 * self.scale), (kind, n)
        assert not np.any(np.abs(nz - LD(TOL_PSD)) <= 1e-9 * self.scale), (kind, n)
        self.rank = int((w > TOL_PSD).sum())     # Jacobi: current_rank
        self.npos = int((w > 0).sum())           # sign: resolved positive eigenvalues
        self.nzero = int((w == 0).sum())         # ... plus at most the unresolved ones
        self.degenerate = kind in ("diagonal", "zero") or not np.any(X64 - np.diag(np.diag(X64)))

    @functools.cached_property
    def s_ref(self):
        return restated_jacobi((self.base or self).X64)[1]


@functools.lru_cache(maxsize=None)
def case(kind, n, tag=0):
    """the case of this kind and side; `tag` separates blocks of equal side"""
    if kind in ("tiny", "huge"):
        b = case("decades", n, tag)
        f = TINY if kind == "tiny" else HUGE
        X = b.X64 * f
        assert np.array_equal(X / f, b.X64)      # an exact power-of-two scaling: the expected value scales with it
        c = Case(kind, n, X, b.ref * LD(f), b.w * LD(f), b.ref_err * f, base=b)
        c.x = b.x * f
        assert np.array_equal(c.x / f, b.x)
        return c
    if kind == "aI_bee":
        a, bb = -1.0, 0.5                        # dyadic: X64 is exact; eigenvalues a (n - 1 times) and a + n b
        X = a * np.eye(n) + bb * np.ones((n, n))
        top = LD(a) + LD(n) * LD(bb)
        w = np.concatenate([np.full(n - 1, LD(a)), [top]]).astype(LD)
        ref = np.full((n, n), max(top, LD(0)) / LD(n), dtype=LD)
        return Case(kind, n, X, ref, w, float(np.finfo(LD).eps) * n)
    rng = np.random.default_rng(_seed(kind, n, tag))
    w = spectrum(kind, n, rng).astype(LD)
    Q = np.eye(n, dtype=LD) if kind == "diagonal" else householder_q(n, rng)
    Xld = (Q * w) @ Q.T
    Xld = (Xld + Xld.T) / LD(2)
    X64 = Xld.astype(np.float64)
    ref = (Q * np.maximum(w, LD(0))) @ Q.T
    ref = (ref + ref.T) / LD(2)
    scale = np.abs(w).max() if n else LD(0)
    orth = np.sqrt(((Q.T @ Q - np.eye(n, dtype=LD)) ** 2).sum())
    err = np.sqrt(((X64.astype(LD) - Xld) ** 2).sum()) + LD(2) * orth * scale
    return Case(kind, n, X64, ref, w, float(err))


# ---------------------------------------------------------------- layouts
def block_table(free):
    """(offsets, sides) of the PSD blocks, offset and length of the SOC, offset of the free variables, n"""
    offs, o = [], 0
    for s in SIDES:
        offs.append(o)
        o += packed_len(s)
    return offs, list(SIDES), (o, SOC_LEN), o + SOC_LEN, o + SOC_LEN + free


def sentinel(n):
    i = np.arange(n, dtype=np.float64)
    return -7.25e300 * (1.0 + (i % 1021.0) / 4096.0)


def deal(d, swap=False):
    """spectrum and case of every PSD block in deal d (None for the 1x1 blocks).  swap: blocks of equal side (the three of
    side 2) trade their data, the first with the last"""
    kinds, j = [], 0
    for s in SIDES:
        if s == 1:
            kinds.append(None)
            continue
        kinds.append((SPECTRA[(j + d) % DEALS], s, j))
        j += 1
    if swap:
        twos = [i for i, s in enumerate(SIDES) if s == 2]
        kinds[twos[0]], kinds[twos[-1]] = kinds[twos[-1]], kinds[twos[0]]
    return [None if k is None else case(*k) for k in kinds]


def one_by_one(d):
    """the two 1x1 blocks: one of each sign, trading places with the deal"""
    v = np.array([-(0.75 + d), 1.25 + d])
    return v if d % 2 == 0 else v[::-1].copy()


def vector(layout, d, swap=False, replace=None):
    """(x, cases): the n-vector of a layout in deal d, in the solver's order (PSD blocks, SOC, free variables)"""
    offs, sides, _, _, n = block_table(LAYOUTS[layout])
    x = sentinel(n)
    cases = deal(d, swap)
    if replace:
        cases = [replace.get(i, c) for i, c in enumerate(cases)]
    ones = iter(one_by_one(d))
    for o, s, c in zip(offs, sides, cases):
        if s == 1:
            x[o] = next(ones)
        else:
            x[o:o + packed_len(s)] = c.x
    return x, cases


def problem(layout):
    """a row-less problem with the layout's cones, variables already in the solver's order"""
    import scipy.sparse as sp
    from proxsdp_jl_amd.problems import Problem
    offs, sides, (so, sl), _, n = block_table(LAYOUTS[layout])
    E = sp.csc_matrix((0, n), dtype=float)
    return Problem(n=n, A=E, b=np.zeros(0), G=E.copy(), h=np.zeros(0), c=np.zeros(n),
                   psd=[np.arange(o, o + packed_len(s), dtype=np.int64) for o, s in zip(offs, sides)],
                   soc=[np.arange(so, so + sl, dtype=np.int64)], name=f"small-blocks-{layout}")


# ---------------------------------------------------------------- the kernel's Jacobi, restated
# A sweep that fails to reduce off^2 by a factor of 10 means "the rounding floor" only where Jacobi converges quadratically.
# Far from convergence a sweep of the cyclic method often gains less (indefinite random input, side 64: off^2 / diag^2 = 12,
# 0.45, 0.078 after 0, 1, 2 sweeps), and stopping there leaves X+ wrong by 3 % to 12 % of the scale.  So a stall counts only
# once off^2 <= 1e-28 diag^2: then off_F <= 1e-14 |A|_F <= 1e-14 sqrt(64) scale, and what the remaining off-diagonal mass can move
# in X+ is below the 1e-13 x scale the Jacobi blocks are held to.  The floors themselves lie at 2e-32 (side 5) .. 5e-31 (side 64).
STALL_REGIME = 1e-28
def round_robin(n):
    """the kernel's schedule: m - 1 rounds of disjoint pairs (p < q) over m = n + (n odd) players; pairs with the dummy dropped"""
    m = n + (n & 1)
    rounds = []
    for rd in range(m - 1):
        pairs = []
        for t in range(m // 2):
            p, q = (m - 1, rd) if t == 0 else ((rd + t) % (m - 1), (rd - t + (m - 1)) % (m - 1))
            if p > q:
                p, q = q, p
            if q < n:
                pairs.append((p, q))
        rounds.append(pairs)
    return rounds


def restated_jacobi(X, max_sweeps=40):
    """Parallel-order cyclic Jacobi as k_small_psd_project runs it, in plain fp64 on a float64 matrix.  Returns
    (ratios, s_ref, A, V): ratios[s] = off^2 / diag^2 after s sweeps; s_ref = the first sweep count s >= 1 after which the
    ratio, at or below STALL_REGIME, failed to fall by a factor of 10 (or reached the kernel's 1e-32 / exact-zero exit); 0 when
    the input is diagonal."""
    n = X.shape[0]
    A, V = np.array(X, dtype=np.float64), np.eye(n)
    rounds = round_robin(n)

    def ratio():
        off = float(np.square(A - np.diag(np.diag(A))).sum())
        dg = float(np.square(np.diag(A)).sum())
        return off, dg
    off, dg = ratio()
    ratios = [off / dg if dg > 0 else (0.0 if off == 0 else np.inf)]
    if off == 0.0 or off <= 1e-32 * dg:
        return ratios, 0, A, V
    s_ref = max_sweeps
    for sweep in range(1, max_sweeps + 1):
        for pairs in rounds:
            if not pairs:
                continue
            P = np.array([p for p, _ in pairs]); Qi = np.array([q for _, q in pairs])
            apq = A[P, Qi]
            c, s = np.ones(len(P)), np.zeros(len(P))
            nzr = apq != 0.0
            with np.errstate(all="ignore"):
                tau = (A[Qi, Qi] - A[P, P])[nzr] / (2.0 * apq[nzr])
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            c[nzr] = 1.0 / np.sqrt(1.0 + t * t)
            s[nzr] = t * c[nzr]
            ap, aq = A[P, :].copy(), A[Qi, :].copy()
            A[P, :] = c[:, None] * ap - s[:, None] * aq
            A[Qi, :] = s[:, None] * ap + c[:, None] * aq
            ap, aq = A[:, P].copy(), A[:, Qi].copy()
            A[:, P] = c * ap - s * aq
            A[:, Qi] = s * ap + c * aq
            vp, vq = V[:, P].copy(), V[:, Qi].copy()
            V[:, P] = c * vp - s * vq
            V[:, Qi] = s * vp + c * vq
        off, dg = ratio()
        ratios.append(off / dg if dg > 0 else 0.0)
        done = off == 0.0 or off <= 1e-32 * dg
        if done or (ratios[-1] <= STALL_REGIME and not ratios[-1] <= 0.1 * ratios[-2]):
            s_ref = sweep
            break
    return ratios, s_ref, A, V
