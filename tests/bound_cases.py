"""Fixtures of the certified dual bound (include/proxsdp_hip.h "a certified dual bound"), all exact in fp64, and the NumPy
side of its checks.  No test here: tests/test_dual_bound_host.py (CPU) and tests/test_dual_bound.py (GPU) use them.

KNOWN OPTIMUM.  Side s, v in {+-1}^s, B = G G' with a small-integer G (s x 3), Z = (s I - v v') B (s I - v v'): an integer
matrix with Z v = 0 and Z >= 0.  With an integer y the model is  min <C, X>, diag X = 1, X >= 0,  C = Z - Diag(y).
SIGNS, settled against k_exit_dual_cone (csrc/exit_device.hip.hpp): the library forms dc = c + M'y and halves the
off-diagonals, so with A = the rows X_ii = 1 and c = (C_ii on a diagonal variable, 2 C_ij on an off-diagonal one) the cone's
matrix of c + A'y_eq at y_eq = +y is C + Diag(y) = Z: the dual is handed in with a PLUS sign, and the dual objective is
-b'y = -sum(y).  X = v v' is feasible with <C, X> = v'Z v - sum(y) = -sum(y), and Z >= 0 makes -sum(y) a lower bound:
p* = -sum(y), an integer known exactly.
Duals fed to the call: y itself, and y + e with a dyadic e: "uniform" (e_i = -eta, eta = 2^-k by the seed: Z~ = Z - eta I has
lambda_min = -eta EXACTLY, and the ideal bound of these duals is again p*) and "seeded" (e_i a seeded multiple of 2^-10 in
[-1, 0]).  Every entry that occurs stays far below 2^53 (asserted in known_optimum), so c, c + A'y and Z~ are exact.

FACTORISATION CASES.  A = L L' with L unit lower triangular ("unit") or with a diagonal in {1, 2, 3} ("scaled"), off-diagonal
entries in {-2 .. 2}: every pivot is a perfect square, every quotient an integer, every partial sum a small integer, so the
factorisation is exact in any order and with fused multiply-adds, and R = L' bit for bit.
"the same matrix minus eps I, eps = 2^-20 tr, must fail by the contrapositive of the theorem" needs lambda_min(A - eps I) <
-delta, which A = L L' does not give by itself (L = I: A - eps I is positive definite).  The unit-triangular L with dense
small-integer entries is so ill-conditioned from side 15 on that it does; indefinite_witness() PROVES it per case in exact
integer arithmetic (an integer x with x'(2^20 A - tr I) x < 0 whose margin exceeds delta x'x), and the sides 1 and 2, where
A - eps I is positive definite, are expected to COMPLETE."""
import numpy as np
import scipy.sparse as sp

from proxsdp_jl_amd import problems as P

U = 2.0 ** -53
FACTOR_SIDES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 257, 449)
BOUND_SIDES_GPU = (17, 65, 257)


def gamma(j):
    return j * U / (1.0 - j * U)


# ---------------------------------------------------------------------------------------------- factorisation cases
def integer_factor(side, seed, kind="unit"):
    """L (float64, integer entries): unit lower triangular, or with a diagonal in {1, 2, 3}"""
    rng = np.random.default_rng(1000 * side + seed)
    L = np.tril(rng.integers(-2, 3, size=(side, side)), -1).astype(np.float64)
    L[np.diag_indices(side)] = 1.0 if kind == "unit" else rng.integers(1, 4, size=side).astype(np.float64)
    return L


def product(L):
    """L L' (exact: small integers)"""
    A = L @ L.T
    assert np.all(A == np.round(A)) and np.abs(A).max() < 2.0 ** 40
    return A


def minus_eps(A):
    """A - eps I, eps = 2^-20 tr A (a dyadic number: the subtraction is exact for these integer matrices)"""
    eps = 2.0 ** -20 * float(np.trace(A))
    return A - eps * np.eye(A.shape[0]), eps


def delta_of(diag, side):
    """delta of a completed factorisation with that diagonal (the header's expression, in plain fp64: the tests add slack)"""
    g = gamma(side + 3)
    return g / (1.0 - g) * float(np.abs(diag).sum()) + U * float(np.abs(diag).max())


def indefinite_witness(A):
    """True when an integer vector x PROVES lambda_min(A - eps I) < -delta, eps = 2^-20 tr A, in exact integer arithmetic:
    x'(2^20 A - tr I) x < -(2^20 delta_up) x'x with delta_up an integer above 2^20 delta.  x: the rounded eigenvector of the
    smallest eigenvalue.  False: no proof (the matrix may still be indefinite)."""
    s = A.shape[0]
    w, V = np.linalg.eigh(A)
    x = np.round(V[:, 0] / np.abs(V[:, 0]).max() * 2.0 ** 20).astype(np.int64)
    xo = x.astype(object)
    Ai = np.round(A).astype(np.int64).astype(object)
    tr = int(round(float(np.trace(A))))
    quad = int(xo @ ((Ai @ xo) * (1 << 20))) - tr * int(xo @ xo)
    delta_up = int(np.ceil(2.0 ** 20 * 2.0 * delta_of(np.diag(A), s))) + 1
    return quad < -delta_up * int(xo @ xo)


def last_pivot_bad(side, seed):
    """(A, L): A = L L' with -1 in place of the last pivot: the first bad pivot sits in the last column, exactly"""
    L = integer_factor(side, seed, "scaled")
    A = product(L)
    A[-1, -1] -= L[-1, -1] ** 2 + 1.0
    return A, L


def spd_real(side, seed):
    """a seeded non-integer symmetric positive definite matrix of moderate condition"""
    rng = np.random.default_rng(7000 * side + seed)
    G = rng.standard_normal((side, side + 3))
    A = G @ G.T / side + 0.25 * np.eye(side)
    return (A + A.T) / 2.0


def assert_backward_error(A, R, what):
    """|R'R - A|_ij <= gamma(s+1) / (1 - gamma(s+1)) sqrt(a_ii a_jj), entry by entry, evaluated in numpy.longdouble: the
    very inequality the certificate assumes"""
    s = A.shape[0]
    Rl, Al = R.astype(np.longdouble), A.astype(np.longdouble)
    E = np.abs(Rl.T @ Rl - Al)
    g = np.longdouble(s + 1) * np.longdouble(U)
    g = g / (1 - g)
    d = np.sqrt(np.diag(Al))
    lim = g / (1 - g) * np.outer(d, d)
    worst = float((E / lim).max())
    print(f"{what}: largest |R'R - A|_ij over its bound = {worst:.3g}")
    assert np.all(E <= lim), (what, worst)


# ---------------------------------------------------------------------------------------------- known optimum
def tri_vector(F):
    """the objective vector of <F, X> on the triangle variables: F_ii on a diagonal, 2 F_ij off it"""
    return P._sym_coeff_vector(np.asarray(F, dtype=np.float64))


def known_optimum(side, seed=0):
    """dict(problem, y (int64), p_star (Python int), Z (float64, integer entries), v)"""
    rng = np.random.default_rng(31 * side + seed)
    v = rng.choice(np.array([-1, 1], dtype=np.int64), size=side)
    G = rng.integers(-2, 3, size=(side, 3)).astype(np.int64)
    Pm = side * np.eye(side, dtype=np.int64) - np.outer(v, v)
    Z = Pm @ (G @ G.T) @ Pm
    y = rng.integers(-5, 6, size=side).astype(np.int64)
    assert np.all(Z @ v == 0) and np.all(Z == Z.T)
    # every number that occurs -- Z, C = Z - Diag(y), 2 C_ij, C_ii + y_i + e_i in units of 2^-10 -- is far below 2^53
    assert 2 * (np.abs(Z).max() + 6) * 2 ** 10 < 2 ** 53
    C = Z - np.diag(y)
    N = P.sympackedlen(side)
    diag = P.tri_index(np.arange(side), np.arange(side))
    A = sp.csc_matrix((np.ones(side), (np.arange(side), diag)), shape=(side, N))
    pr = P.Problem(n=N, A=A, b=np.ones(side), G=P._empty(N), h=np.zeros(0), c=tri_vector(C),
                   psd=[np.arange(N, dtype=np.int64)], name=f"known-optimum-{side}-{seed}")
    return dict(problem=pr, y=y, p_star=-int(y.sum()), Z=Z.astype(np.float64), v=v, side=side)


def duals(case, kind, seed=0):
    """(dual_eq, Z~, lambda_min or None): kind "exact" (y), "uniform" (y - eta 1), "seeded" (y + a seeded dyadic e <= 0)"""
    s, y, Z = case["side"], case["y"].astype(np.float64), case["Z"]
    if kind == "exact":
        return y, Z.copy(), 0.0
    if kind == "uniform":
        eta = 2.0 ** -(2 + 3 * ((s + seed) % 3))
        return y - eta, Z - eta * np.eye(s), -eta
    rng = np.random.default_rng(977 * s + seed)
    e = -rng.integers(0, 1025, size=s).astype(np.float64) / 1024.0
    return y + e, Z + np.diag(e), None


# ---------------------------------------------------------------------------------------------- the NumPy side of the checks
def dual_matrices(pr, dual_eq, dual_in):
    """the cones' matrices of c + A'y_eq + G'max(y_in, 0), off-diagonals halved (plain NumPy, rounding as it comes)"""
    t = np.asarray(pr.c, dtype=np.float64).copy()
    if pr.A.shape[0]:
        t = t + pr.A.T @ np.asarray(dual_eq, dtype=np.float64)
    if pr.G.shape[0]:
        t = t + pr.G.T @ np.maximum(np.asarray(dual_in, dtype=np.float64), 0.0)
    out = []
    for idx, s in zip(pr.psd, pr.psd_sides()):
        Zm = np.zeros((s, s))
        jj = np.repeat(np.arange(s), np.arange(1, s + 1))
        ii = np.concatenate([np.arange(j + 1) for j in range(s)])
        Zm[ii, jj] = t[idx] / 2.0
        Zm = Zm + Zm.T
        out.append(Zm)
    return out


def assert_tight(db, k, Zt, what):
    """the issue's tightness rule for cone k against the ideal bound of the same duals: with lam = eigvalsh(Z~).min(),
    sigma* lies within 0.1 |min(0, lam)| + 4 (delta + nu 2^-48) of max(0, -lam).  0.1 is the search's resolution
    (16^(1/32) - 1 < 0.1), the rest are the certificate's own terms; nothing is a measured number."""
    assert db.certified[k], what
    lam = float(np.linalg.eigvalsh(Zt).min())
    nu = float(np.abs(Zt).sum(axis=1).max())
    delta = float(db.delta[k])
    slack = 0.1 * abs(min(0.0, lam)) + 4.0 * (delta + nu * 2.0 ** -48)
    print(f"{what}: lambda_min {lam:.6g}, sigma* {db.shift[k]:.6g}, delta {delta:.3g}, rho {db.radius[k]:.3g}, "
          f"tries {db.factorisations[k]}, allowed distance {slack:.3g}")
    assert abs(float(db.shift[k]) - max(0.0, -lam)) <= slack, (what, db.shift[k], lam, slack)
    # delta is the header's expression at sigma* (the library rounds it up: a few ulps above the plain evaluation)
    want = delta_of(np.diag(Zt) + db.shift[k], Zt.shape[0])
    assert want * (1 - 1e-12) <= delta <= want * (1 + 1e-12), (what, delta, want)
    assert db.lambda_lower[k] <= -(db.shift[k] + delta + db.radius[k]) * (1 - 1e-15)
    assert db.lambda_lower[k] >= -(db.shift[k] + delta + db.radius[k]) * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------- Max-Cut with triangle rows
def maxcut16_with_triangles(seed=0, rows=40):
    """P.maxcut(16) with `rows` seeded triangle inequalities (valid for every cut matrix) as G x <= h, and the largest cut by
    brute force over the 2^15 sign vectors"""
    n = 16
    L = P.erdos_renyi_laplacian(n, seed, 6.0)
    pr = P.maxcut_from_laplacian(L, name="maxcut16-triangles")
    Ld = np.asarray(L.todense()) if sp.issparse(L) else np.asarray(L)
    rng = np.random.default_rng(seed + 5)
    signs = np.array([(-1, -1, -1), (-1, 1, 1), (1, -1, 1), (1, 1, -1)], dtype=np.float64)
    r_i, c_i, vals = [], [], []
    for r in range(rows):
        i, j, k = np.sort(rng.choice(n, size=3, replace=False))
        sg = signs[rng.integers(0, 4)]
        for (a, b), sv in zip(((i, j), (i, k), (j, k)), sg):
            r_i.append(r); c_i.append(int(P.tri_index(a, b))); vals.append(sv)
    G = sp.csc_matrix((vals, (r_i, c_i)), shape=(rows, pr.n))
    import dataclasses
    pr = dataclasses.replace(pr, G=G, h=np.ones(rows))
    bits = np.arange(1 << (n - 1), dtype=np.int64)
    X = np.where((bits[:, None] >> np.arange(n - 1)[None, :]) & 1, 1.0, -1.0)
    X = np.concatenate([X, np.ones((len(bits), 1))], axis=1)
    best = float((0.25 * np.einsum("ti,ij,tj->t", X, Ld, X)).max())
    return pr, best
