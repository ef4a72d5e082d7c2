"""Fixtures and the NumPy restatement of the rounding tests (test_rounding_host.py, test_rounding.py).

The restatement restates the contract of include/proxsdp_hip.h ("rounding on a model handle") and nothing else, vectorised
over the trials only: it loops over the columns k, over the nodes and over a node's neighbours in the contract's order, so
every fp64 expression is evaluated left to right as written (NumPy does not contract).  The generator is oracle/eig.py's
(the mirror of csrc/host_util.hpp).  No library source is read."""
import functools

import numpy as np

from oracle.eig import _uniform53


# ---------------------------------------------------------------- the contract, restated
def directions(seed, r, trials):
    """g (r x trials): g(k, t) = (((u_0 + u_1) + ... + u_11) - 6.0), u_q = uniform53(seed, (t r + k) 12 + q)"""
    t = np.arange(trials, dtype=np.uint64)[None, :]
    k = np.arange(r, dtype=np.uint64)[:, None]
    base = (t * np.uint64(r) + k) * np.uint64(12)
    z = _uniform53(seed, base)
    for q in range(1, 12):
        z = z + _uniform53(seed, base + np.uint64(q))
    return z - 6.0


def tri(i, j):
    i, j = min(i, j), max(i, j)
    return j * (j + 1) // 2 + i


def adjacency(cc, s):
    """(ptr, cols, values, diag) of a cone's part of c (upper triangle column by column): d_i = c[var(i, i)], adj(i) = the
    j != i with c[var(i, j)] != 0, ascending"""
    cc = np.asarray(cc, dtype=np.float64)
    W = np.zeros((s, s))
    for j in range(s):
        W[:j + 1, j] = cc[j * (j + 1) // 2:j * (j + 1) // 2 + j + 1]
    diag = np.diag(W).copy()
    W = W + W.T
    np.fill_diagonal(W, 0.0)
    ptr, cols, vals = [0], [], []
    for i in range(s):
        nz = np.nonzero(W[i] != 0.0)[0]
        cols.extend(nz.tolist())
        vals.extend(W[i, nz].tolist())
        ptr.append(len(cols))
    return (np.array(ptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64), diag)


def values_of(sg, adj):
    """the value of every column of sg (s x T, +-1.0), in the contract's order"""
    ptr, cols, vals, diag = adj
    s, T = sg.shape
    f = np.zeros(T)
    for i in range(s):
        f = f + diag[i]
    for i in range(s):
        u = np.zeros(T)
        for e in range(ptr[i], ptr[i + 1]):
            if cols[e] > i:
                u = u + vals[e] * sg[cols[e]]
        f = f + sg[i] * u
    return f


def restate(values, V, adj, trials, seed, max_sweeps):
    """every output of the contract as a dictionary: signs (int8), best_trial, value, value_rounded, values_rounded,
    values_final, sweeps, flips"""
    ptr, cols, vals, diag = adj
    values, V = np.asarray(values, dtype=np.float64), np.asarray(V, dtype=np.float64)
    s, r = V.shape
    w = np.sqrt(values)
    g = directions(seed, r, trials)
    y = np.zeros((s, trials))
    for k in range(r):
        y = y + (V[:, k] * w[k])[:, None] * g[k][None, :]
    sg = np.where(y < 0.0, -1.0, 1.0)
    rounded = values_of(sg, adj)
    active = np.ones(trials, dtype=bool)                           # trials whose last sweep flipped something
    sweeps = np.zeros(trials, dtype=np.int64)
    flips = 0
    for _ in range(max_sweeps):
        if not active.any():
            break
        sweeps[active] += 1
        flipped = np.zeros(trials, dtype=bool)
        for i in range(s):
            a = np.zeros(trials)
            for e in range(ptr[i], ptr[i + 1]):
                a = a + vals[e] * sg[cols[e]]
            fl = (sg[i] * a > 0.0) & active
            sg[i, fl] = -sg[i, fl]
            flipped |= fl
            flips += int(fl.sum())
        active &= flipped
    final = values_of(sg, adj)
    best = int(np.argmin(final))                                   # (the first of equal minima)
    return dict(signs=sg[:, best].astype(np.int8), best_trial=best, value=float(final[best]), value_rounded=float(rounded.min()),
                values_rounded=rounded, values_final=final, sweeps=int(sweeps.max()), flips=flips)


OUTPUTS = ("signs", "best_trial", "value", "value_rounded", "values_rounded", "values_final", "sweeps", "flips")


def assert_rounding_equal(got, want, what):
    """a binding.Rounding against restate(): every output, exactly"""
    for k in OUTPUTS:
        a, b = getattr(got, k), want[k]
        if isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, k)
        else:
            assert a == b, (what, k, a, b)


def cone_value(cc, signs):
    """the cone's part of c'x at x = the triangle of sigma sigma', by one NumPy dot (exact for dyadic weights)"""
    sg = np.asarray(signs, dtype=np.float64)
    s = len(sg)
    x = np.concatenate([sg[:j + 1] * sg[j] for j in range(s)])
    return float(np.dot(np.asarray(cc, dtype=np.float64), x))


def brute_force_minimum(cc, s):
    """the smallest value over all sign vectors (sigma_0 = +1: the value is even in sigma); dyadic weights only, where every
    order of summation gives the same number"""
    ptr, cols, vals, diag = adjacency(cc, s)
    W = np.zeros((s, s))
    for i in range(s):
        W[i, cols[ptr[i]:ptr[i + 1]]] = vals[ptr[i]:ptr[i + 1]]
    bits = (np.arange(1 << (s - 1))[:, None] >> np.arange(s - 1)[None, :]) & 1
    sg = np.concatenate([np.ones((len(bits), 1)), np.where(bits == 1, -1.0, 1.0)], axis=1)
    return float((diag.sum() + 0.5 * np.einsum("ti,ij,tj->t", sg, W, sg)).min())


# ---------------------------------------------------------------- fixtures
def pack(W, diag):
    """a cone's part of c (upper triangle column by column) from the symmetric off-diagonal weights W and the diagonal"""
    s = len(diag)
    M = np.array(W, dtype=np.float64)
    np.fill_diagonal(M, diag)
    return np.concatenate([M[:j + 1, j] for j in range(s)])


def graph(s, seed, degree=4.0, kind="dyadic", isolated=()):
    """the cone's part of c of a seeded G(s, p), p = degree / (s - 1).  dyadic: the Max-Cut model's numbers, an edge of weight
    +-1 gives w_ij = +-0.5 and d_i = -0.25 (the sum of the node's edge weights); real: w_ij and d_i standard normal.  The
    nodes of `isolated` lose every edge."""
    rng = np.random.default_rng(seed)
    p = min(1.0, degree / max(s - 1, 1))
    E = np.triu(rng.random((s, s)) < p, 1)
    if s >= 2 and not E.any():
        E[0, 1] = True                                             # (a graph with no edge at all is zero_c's business)
    if kind == "dyadic":
        Wt = np.where(E, np.where(rng.random((s, s)) < 0.25, -1.0, 1.0), 0.0)
    else:
        Wt = np.where(E, rng.standard_normal((s, s)), 0.0)
    Wt = Wt + Wt.T
    for i in isolated:
        Wt[i, :] = 0.0
        Wt[:, i] = 0.0
    if kind == "dyadic":
        return pack(0.5 * Wt, -0.25 * Wt.sum(axis=1))
    return pack(Wt, rng.standard_normal(s))


def zero_c(s):
    return np.zeros(s * (s + 1) // 2)


@functools.lru_cache(maxsize=None)
def _factors(s, r, seed):
    G = np.random.default_rng(seed).standard_normal((s, r))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    lam, U = np.linalg.eigh(G @ G.T)
    lam, U = lam[::-1][:r], U[:, ::-1][:, :r]
    assert np.all(lam > 0.0)
    return lam, U


def factors(s, r, seed=0):
    """(values (r,) descending and > 0, vectors (s, r)): the leading r eigenpairs of G G' for a seeded s x r Gaussian G with
    rows normalised to unit length"""
    lam, U = _factors(s, r, seed)
    return lam.copy(), np.ascontiguousarray(U)
