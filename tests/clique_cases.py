"""Fixtures and the NumPy restatement of the pentagonal / heptagonal separation tests (test_clique_cuts_host.py,
test_clique_cuts.py).

The restatement states the contract of include/proxsdp_hip.h ("pentagonal and heptagonal cuts") and nothing else: per base
B and t in the written association, the four codes as whole matrices ((B - tau_l t[:, None]) - tau_m t[None, :]) -
(tau_l tau_m) X) - rhs (a product with +-1.0 is exact), the first maximum in the order (l, m, code), then normal form, merge,
sort and the emitted rows.  The GPU source is read for constants only (the tile of the sweep), never for expected values."""
import itertools
import pathlib
import re

import numpy as np

from triangle_cases import feasible, gram, pack, ties, tri_index  # noqa: F401  (the fixtures the tests share)

SOURCE = pathlib.Path(__file__).resolve().parent.parent / "proxsdp.jl_amd" / "csrc" / "clique_cuts.hip.hpp"
CODES = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))        # code: (tau_l, tau_m)
PATTERN_SIGNS = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]], dtype=np.int8)   # of a triangle row's pattern


def sweep_tile():
    """CLQ_TILE of csrc/clique_cuts.hip.hpp: the side of a tile of (l, m) pairs"""
    return int(re.search(r"constexpr int CLQ_TILE = (\d+);", SOURCE.read_text()).group(1))


def sweep_wave():
    """CLQ_WAVE of csrc/clique_cuts.hip.hpp: the bases of one workgroup of the sweep"""
    return int(re.search(r"constexpr int CLQ_WAVE = (\d+);", SOURCE.read_text()).group(1))


# ---------------------------------------------------------------- fixtures
def planted(side, nodes, seed=0):
    """gram(side, 3, seed) with the five `nodes` replaced by the unit vectors at the angles 2 pi 2 k / 5 of the plane: they sum
    to zero, so the pentagon on them with signs (+,+,+,+,+) has -sum X_ab - 2 = 0.5, the most a PSD matrix allows"""
    V = np.random.default_rng(seed).standard_normal((side, 3))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    for k, a in enumerate(nodes):
        V[a] = [np.cos(4.0 * np.pi * k / 5.0), np.sin(4.0 * np.pi * k / 5.0), 0.0]
    return V @ V.T


def bases_from_triangles(want, n_base=None):
    """(nodes, signs) of the first n_base rows of a triangle_cases.brute_force dictionary"""
    k = want["n_rows"] if n_base is None else n_base
    assert k <= want["n_rows"]
    return want["tri"][:k].astype(np.int64), PATTERN_SIGNS[want["pattern"][:k]]


def all_triangles(side):
    """every triple with every sign pattern whose first sign is +1: 4 C(side, 3) bases"""
    T = np.array(list(itertools.combinations(range(side), 3)), dtype=np.int64)
    return np.repeat(T, 4, axis=0), np.tile(PATTERN_SIGNS, (len(T), 1))


# ---------------------------------------------------------------- the restatement
def _sym(X):
    """the matrix the library sees: the strict upper triangle mirrored (the diagonal is never read)"""
    U = np.triu(np.asarray(X, dtype=np.float64), 1)
    return U + U.T


def extend(X, nodes, signs, rhs):
    """(v, l, m, code) of the best extension of one base; X symmetric"""
    s = X.shape[0]
    a, sg = [int(x) for x in nodes], [float(x) for x in signs]
    B = None
    for u in range(len(a)):
        for w in range(u + 1, len(a)):
            term = (-sg[u] * sg[w]) * X[a[u], a[w]]
            B = term if B is None else B + term
    t = sg[0] * X[a[0], :]
    for u in range(1, len(a)):
        t = t + sg[u] * X[a[u], :]
    t = t.copy()
    t[a] = np.nan
    V = np.stack([(((B - tl * t[:, None]) - tm * t[None, :]) - (tl * tm) * X) - rhs for tl, tm in CODES], axis=2)
    V[np.tril_indices(s)] = np.nan                                   # l < m only
    V = np.where(np.isnan(V), -np.inf, V)
    flat = int(np.argmax(V))                                         # the FIRST maximum in the order (l, m, code)
    l, m, code = flat // (4 * s), (flat // 4) % s, flat % 4
    return float(V[l, m, code]), l, m, code


def restatement(X, bases, min_violation=1e-3, rhs=None, cone_idx=None, index_base=0):
    """what the separation must return, as a dictionary of the fields the tests compare"""
    X = _sym(X)
    s = X.shape[0]
    nodes, signs = np.asarray(bases[0], dtype=np.int64), np.asarray(bases[1], dtype=np.int8)
    nb, q = nodes.shape
    k = q + 2
    rhs = (q + 1) / 2 if rhs is None else rhs
    found = {}                                                       # (nodes, signs) -> (v, base)
    values = np.zeros(nb)
    for b in range(nb):
        v, l, m, code = extend(X, nodes[b], signs[b], rhs)
        values[b] = v
        if not v > min_violation:
            continue
        both = sorted(list(zip(nodes[b].tolist(), signs[b].tolist())) + [(l, int(CODES[code][0])), (m, int(CODES[code][1]))])
        nn, ss = tuple(x for x, _ in both), tuple(y * both[0][1] for _, y in both)
        old = found.get((nn, ss))
        if old is None or v > old[0]:                                # (equal v: the lower base, which came first, stays)
            found[(nn, ss)] = (v, b)
    violated = int((values > min_violation).sum())
    rows = sorted(((-v, b, nn, ss) for (nn, ss), (v, b) in found.items()))
    n = len(rows)
    out_nodes = np.array([r[2] for r in rows], dtype=np.int64).reshape(n, k)
    out_signs = np.array([r[3] for r in rows], dtype=np.int8).reshape(n, k)
    pairs = list(itertools.combinations(range(k), 2))
    pos = np.array([[tri_index(r[u], r[w]) for u, w in pairs] for r in out_nodes], dtype=np.int64).reshape(n, len(pairs))
    col = pos + index_base if cone_idx is None else np.asarray(cone_idx, dtype=np.int64)[pos]
    val = np.array([[-float(r[u]) * float(r[w]) for u, w in pairs] for r in out_signs]).reshape(n, len(pairs))
    return dict(nodes=out_nodes, signs=out_signs, violation=np.array([-r[0] for r in rows]),
                from_base=np.array([r[1] for r in rows], dtype=np.int64), add_col=col.reshape(-1), add_val=val.reshape(-1),
                add_h=np.full(n, float(rhs)), n_rows=n, violated_bases=violated,
                scanned=nb * 4 * ((s - q) * (s - q - 1) // 2), values=values, size=k)


def assert_cliques_equal(cuts, want, what, raw_base=None):
    """a binding.CliqueCuts against restatement's dictionary, exactly"""
    assert len(cuts) == want["n_rows"] and cuts.violated_bases == want["violated_bases"] and cuts.scanned == want["scanned"], \
        (what, len(cuts), want["n_rows"], cuts.violated_bases, want["violated_bases"], cuts.scanned, want["scanned"])
    assert cuts.size == want["size"] and cuts.nodes.shape == want["nodes"].shape, (what, "shape")
    assert np.array_equal(cuts.nodes, want["nodes"]) and cuts.nodes.dtype == np.int64, (what, "nodes")
    assert np.array_equal(cuts.signs, want["signs"]) and cuts.signs.dtype == np.int8, (what, "signs")
    assert np.array_equal(cuts.violations, want["violation"]), (what, "violation")
    assert np.array_equal(cuts.from_base, want["from_base"]), (what, "from_base")
    assert np.array_equal(cuts.raw["add_col"], want["add_col"]), (what, "add_col")
    assert np.array_equal(cuts.raw["add_val"], want["add_val"]), (what, "add_val")
    assert np.array_equal(cuts.raw["add_h"], want["add_h"]), (what, "add_h")
    (ptr, cols, vals), h = cuts.add
    k = want["size"]
    assert np.array_equal(ptr, (k * (k - 1) // 2) * np.arange(len(cuts) + 1)), (what, "rowptr")
    if raw_base is not None:
        assert np.array_equal(cols, want["add_col"] - raw_base), (what, "cols")


def lhs(X, nodes, signs):
    """the left side of a row at X: sum over pairs of -sigma_u sigma_w X[n_u, n_w]"""
    return sum(-float(signs[u]) * float(signs[w]) * X[nodes[u], nodes[w]] for u, w in itertools.combinations(range(len(nodes)), 2))
