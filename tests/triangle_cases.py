"""Fixtures and the NumPy brute force of the triangle separation tests (test_triangle_cuts_host.py, test_triangle_cuts.py).

The brute force restates the contract of include/proxsdp_hip.h ("separation on a model handle") and nothing else: every
triple of itertools.combinations, the four patterns, v = ((s1 X_ij + s2 X_ik) + s3 X_jk) - rhs in fp64 in this association
(a product with +-1.0 is exact), the rows with v > min_violation sorted by (-v, i, j, k, pattern).  The GPU source is read
for constants only (the tile of the sweep), never for expected values."""
import functools
import itertools
import pathlib
import re

import numpy as np

SIGNS = np.array([[-1.0, -1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0]])
SOURCE = pathlib.Path(__file__).resolve().parent.parent / "proxsdp.jl_amd" / "csrc" / "triangle_cuts.hip.hpp"


def sweep_tile():
    """TRI_TILE of csrc/triangle_cuts.hip.hpp: the side of a workgroup's (i, j) tile and the length of a chunk of k"""
    return int(re.search(r"constexpr int TRI_TILE = (\d+);", SOURCE.read_text()).group(1))


# ---------------------------------------------------------------- fixtures
def gram(side, r, seed):
    """rows of a standard-normal side x r matrix normalised to unit length; X = V V'"""
    V = np.random.default_rng(seed).standard_normal((side, r))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    return V @ V.T


def ties(side):
    """X = 1.5 I - 0.5 ones: every pattern-0 row has v = 0.5 exactly (rhs = 1), no other pattern is violated"""
    return 1.5 * np.eye(side) - 0.5 * np.ones((side, side))


def feasible(side, seed=0):
    """X = x x' for a +-1 vector: a cut matrix violates nothing"""
    x = np.where(np.random.default_rng(seed).standard_normal(side) < 0, -1.0, 1.0)
    return np.outer(x, x)


def tri_index(i, j):
    """position of X_ij, i <= j, in the upper triangle stored column by column"""
    return j * (j + 1) // 2 + i


def pack(X):
    """the upper triangle of X column by column: a cone's entries in the order of its variable list"""
    s = X.shape[0]
    return np.array([X[i, j] for j in range(s) for i in range(j + 1)])


# ---------------------------------------------------------------- the brute force
@functools.lru_cache(maxsize=None)
def _triples(side):
    T = np.array(list(itertools.combinations(range(side), 3)), dtype=np.int64).reshape(-1, 3)
    T.setflags(write=False)
    return T


def all_rows(X, rhs=1.0):
    """(triples, violations): row t of triples against the 4 columns of violations, one per pattern"""
    X = np.asarray(X, dtype=np.float64)
    T = _triples(X.shape[0])
    a, b, c = X[T[:, 0], T[:, 1]], X[T[:, 0], T[:, 2]], X[T[:, 1], T[:, 2]]
    V = np.stack([((s[0] * a + s[1] * b) + s[2] * c) - rhs for s in SIGNS], axis=1)
    return T, V


def brute_force(X, count, min_violation=1e-3, rhs=1.0, cone_idx=None, index_base=0):
    """what the separation must return, as a dictionary of the fields the tests compare"""
    T, V = all_rows(X, rhs)
    t, p = np.nonzero(V > min_violation)
    v = V[t, p]
    order = np.lexsort((p, T[t, 2], T[t, 1], T[t, 0], -v))[:count]
    t, p, v = t[order], p[order], v[order]
    tri = T[t]
    pairs = [(tri[:, 0], tri[:, 1]), (tri[:, 0], tri[:, 2]), (tri[:, 1], tri[:, 2])]
    pos = np.stack([tri_index(i, j) for i, j in pairs], axis=1).reshape(-1, 3)
    col = pos + index_base if cone_idx is None else np.asarray(cone_idx, dtype=np.int64)[pos]
    return dict(tri=tri.reshape(-1, 3), pattern=p.astype(np.int32), violation=v, add_col=col.reshape(-1), add_val=SIGNS[p].reshape(-1),
                add_h=np.full(len(v), float(rhs)), n_rows=len(v), violated=int((V > min_violation).sum()),
                scanned=4 * len(T))


def assert_cuts_equal(cuts, want, what, raw_base=None):
    """a binding.TriangleCuts against brute_force's dictionary, exactly"""
    assert len(cuts) == want["n_rows"] and cuts.violated == want["violated"] and cuts.scanned == want["scanned"], \
        (what, len(cuts), want["n_rows"], cuts.violated, want["violated"], cuts.scanned, want["scanned"])
    assert np.array_equal(cuts.triples, want["tri"]), (what, "tri")
    assert np.array_equal(cuts.patterns, want["pattern"]) and cuts.patterns.dtype == np.int32, (what, "pattern")
    assert np.array_equal(cuts.violations, want["violation"]), (what, "violation")
    assert np.array_equal(cuts.raw["add_col"], want["add_col"]), (what, "add_col")
    assert np.array_equal(cuts.raw["add_val"], want["add_val"]), (what, "add_val")
    assert np.array_equal(cuts.raw["add_h"], want["add_h"]), (what, "add_h")
    (ptr, cols, vals), h = cuts.add
    assert np.array_equal(ptr, 3 * np.arange(len(cuts) + 1)), (what, "rowptr")
    if raw_base is not None:
        assert np.array_equal(cols, want["add_col"] - raw_base), (what, "cols")
