"""Shared builders of the row-change tests (test_model_rows_host.py, test_model_rows.py): triangle inequalities on a Max-Cut
relaxation, the models with duplicate entries, and a hand-built stacker that realises the storage order
proxsdp_hip_model_rows documents -- column by column, a column's kept entries in the order they are stored now, then its
new entries by ascending new row, the entries of one row and column in the order the row lists them."""
import itertools

import numpy as np
import scipy.sparse as sp

from proxsdp_jl_amd import problems as P

TRIANGLE_SIGNS = ((-1.0, -1.0, -1.0), (-1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, -1.0))


def triangle_rows(side, triples):
    """The four triangle inequalities of every triple (i, j, k) of a side x side Max-Cut relaxation as CSR arrays over its
    packed triangle: (rowptr, cols, values), h.  Row 4 q + s has the entries TRIANGLE_SIGNS[s] on X_ij, X_ik, X_jk, h = 1."""
    ptr, cols, vals = [0], [], []
    for i, j, k in triples:
        cc = [int(P.tri_index(i, j)), int(P.tri_index(i, k)), int(P.tri_index(j, k))]
        for sg in TRIANGLE_SIGNS:
            cols += cc
            vals += list(sg)
            ptr.append(len(cols))
    assert side * (side + 1) // 2 > max(cols, default=0)
    return (np.array(ptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)), np.ones(len(ptr) - 1)


def all_triples(side):
    return list(itertools.combinations(range(side), 3))


def first_triples(side, count):
    return list(itertools.islice(itertools.combinations(range(side), 3), count))


def csc_parts(M):
    """(indptr, indices, data) of a matrix in sorted CSC storage, duplicates kept (what the binding hands the library)"""
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.copy()


def stack_rows(G, h, add=None, drop=()):
    """G' = [the rows of G not in drop, in their old order; the new rows], h' likewise, built entry by entry in the documented
    storage order.  Returns (G' as a csc_matrix whose stored order IS that order, h', kept, src) with src[q] = where stored
    entry q of G' comes from: q0 >= 0 = stored entry q0 of G, -1 - t = entry t of the new values."""
    indptr, indices, data = csc_parts(G)
    m, n = G.shape
    drop = set(int(r) for r in (drop if drop is not None else ()))
    newrow, kept = {}, []
    for r in range(m):
        if r not in drop:
            newrow[r] = len(kept)
            kept.append(r)
    mk = len(kept)
    cols_new = [[] for _ in range(n)]                         # per column: (new row, t) in ascending row, then listed order
    k_add = 0
    h2 = [float(h[r]) for r in kept]
    vals = np.zeros(0)
    if add is not None:
        (ptr, cols, vals), h_new = add
        k_add = len(ptr) - 1
        for r in range(k_add):
            for t in range(int(ptr[r]), int(ptr[r + 1])):
                cols_new[int(cols[t])].append((mk + r, t))
        h2 += [float(v) for v in h_new]
        kept = kept + [-1] * k_add
    ip, ix, dat, src = [0], [], [], []
    for j in range(n):
        for q in range(int(indptr[j]), int(indptr[j + 1])):
            r = int(indices[q])
            if r in newrow:
                ix.append(newrow[r]); dat.append(data[q]); src.append(q)
        for r, t in cols_new[j]:
            ix.append(r); dat.append(float(vals[t])); src.append(-1 - t)
        ip.append(len(ix))
    G2 = sp.csc_matrix((np.array(dat, dtype=np.float64), np.array(ix, dtype=np.int32), np.array(ip, dtype=np.int32)),
                       shape=(mk + k_add, n))
    # (sorted CSC storage keeps this order: inside a column the rows already ascend, ties in listed order)
    assert all(np.all(np.diff(G2.indices[ip[j]:ip[j + 1]]) >= 0) for j in range(n))
    return G2, np.array(h2), np.array(kept, dtype=np.int64), np.array(src, dtype=np.int64)


def with_rows(pr, G2, h2):
    return P.Problem(n=pr.n, A=pr.A, b=pr.b, G=G2, h=h2, c=pr.c, psd=pr.psd, soc=pr.soc, max_sense=pr.max_sense,
                     objective_constant=pr.objective_constant)


def random_with_duplicates(seed):
    """tests/test_model_handle_host.py's model, restated: two PSD cones (and a 1x1), one SOC and free variables, the variables
    not in solver order, and columns of A and G that store the same row more than once"""
    rng = np.random.default_rng(seed)
    sides = (3, 1, 4)
    lens = [s * (s + 1) // 2 for s in sides]
    n = sum(lens) + 3 + 2
    perm = rng.permutation(n)
    psd, pos = [], 0
    for ln in lens:
        psd.append(perm[pos:pos + ln].astype(np.int64)); pos += ln
    soc = [perm[pos:pos + 3].astype(np.int64)]

    def mat(rows):
        indptr, indices = [0], []
        for j in range(n):
            cnt = int(rng.integers(0, 4))
            r = rng.integers(0, rows, cnt)
            if cnt >= 2 and rng.random() < 0.5:
                r[1] = r[0]                                        # a duplicate inside the column
            indices += sorted(int(v) for v in r)
            indptr.append(len(indices))
        data = rng.standard_normal(len(indices))
        return sp.csc_matrix((data, np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(rows, n))

    A, G = mat(5), mat(4)
    assert not A.has_canonical_format or not G.has_canonical_format, "the pattern has no duplicate"
    c = rng.standard_normal(n) * (rng.random(n) < 0.7)
    return P.Problem(n=n, A=A, b=rng.standard_normal(5), G=G, h=rng.standard_normal(4), c=c, psd=psd, soc=soc)


def duplicate_rows(n, seed):
    """three new rows over n variables: one that lists a column twice, one empty, one plain"""
    rng = np.random.default_rng(100 + seed)
    c0 = rng.choice(n, size=3, replace=False)
    c2 = rng.choice(n, size=4, replace=False)
    cols = np.array([c0[0], c0[1], c0[0], c0[2]] + list(c2), dtype=np.int64)      # row 0 lists c0[0] twice; row 1 is empty
    ptr = np.array([0, 4, 4, 8], dtype=np.int64)
    return (ptr, cols, rng.standard_normal(8)), rng.standard_normal(3)


def c5():
    """Max-Cut on the unit-weight 5-cycle"""
    L = np.zeros((5, 5))
    for i in range(5):
        j = (i + 1) % 5
        L[i, i] += 1; L[j, j] += 1; L[i, j] -= 1; L[j, i] -= 1
    return P.maxcut_from_laplacian(L, name="maxcut-c5")
