"""Fixtures and expected values for the device exit path (csrc/exit_device.hip.hpp; proxsdp_hip_exit_vectors,
proxsdp_hip_solve_device).

`expected(case)` restates cache_solution + get_duals + dual_feas (pdhg.jl:678-787) as the library's host path orders them, in
plain Python float arithmetic (IEEE double, no fused multiply-add), one operation at a time:

  x          off-diagonal PSD entries times 1 / sqrt(2) (the in-place fix_diag_scaling of the iterate)
  slack[r]   acc = 0; acc += val * x[k] over the entries of row r in ascending solver-order column k (a column's own entries
             in storage order); then acc - b[r] (or h)
  dc[k]      acc = 0; acc += val * y[row] over the entries of column k in storage order; then c[k] + acc; then / 2.0 where
             the entry is an off-diagonal PSD entry
  primal[i] = x[inv[i]], dual_cone[i] = dc[inv[i]]; the duals are y's two halves
  viol       -min(0, min y_in) | max(0, -min(0, min of dc over the 1x1 cones)) | the same over dc[0] - sqrt(sum dc[i]^2) of
             every second-order cone, the sum in index order | max |dc| over the variables outside every cone
  neg        minus the dual-cone block of every PSD cone of side >= 2, in cone order

The solver's variable order comes from B.host_preprocess (cone variables first, in cone order); nothing else of the library is
used.  Matrix entries and iterates are full-mantissa random numbers, so a sum taken in another order differs in its last bits
(`expected(case, reverse_col=k, reverse_row=r)` takes one column's and one row's sum backwards: the host tests use it to show
that the fixtures can tell).

The kernels run one thread per column and one per row at every length, so there is no length at which a kernel changes form
and no case on either side of one.  The dense case is the exception to "full mantissa": the dense products A x and c + A'y are
dense_mv's and dense_mtv's, whose own summation order is theirs (and tested where they are); its iterate has ONE non-zero
entry in x and one in y_eq, each a power of two, so those two products are exact in any order, while G'y_in on top of them is
a sum of full-mantissa terms.
"""
import math
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P


@dataclass
class Case:
    name: str
    prob: object
    x: np.ndarray            # internal iterate, solver order and scale (n)
    y: np.ndarray            # internal dual (p + m)
    zero_c: bool = False
    index_base: int = 0
    long_col: int = -1       # a solver-order column / a row with at least three entries (-1: the case has none)
    long_row: int = -1


def _csc(rows, cols, vals, shape):
    """CSC with the entries as given, duplicates kept (scipy would sum them on conversion from COO)"""
    order = np.lexsort((np.arange(len(rows)), rows, cols))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals, float)[order]
    indptr = np.zeros(shape[1] + 1, dtype=np.int64)
    np.add.at(indptr, cols + 1, 1)
    return sp.csc_matrix((vals, rows.astype(np.int64), np.cumsum(indptr)), shape=shape)


def _iterate(rng, n, Q):
    return rng.standard_normal(n), rng.standard_normal(Q)


def case_one_equality():
    rng = np.random.default_rng(101)
    pr = P.Problem(n=1, A=sp.csc_matrix(rng.standard_normal((1, 1))), b=rng.standard_normal(1),
                   G=sp.csc_matrix((0, 1)), h=np.zeros(0), c=rng.standard_normal(1), name="one-equality")
    return Case("one_equality", pr, *_iterate(rng, 1, 1))


def case_one_inequality():
    rng = np.random.default_rng(102)
    pr = P.Problem(n=1, A=sp.csc_matrix((0, 1)), b=np.zeros(0), G=sp.csc_matrix(rng.standard_normal((1, 1))),
                   h=rng.standard_normal(1), c=rng.standard_normal(1), name="one-inequality")
    return Case("one_inequality", pr, *_iterate(rng, 1, 1))


def _mixed_problem():
    """12 variables in a scrambled user order: free 0, 7 | SOC (3) 4, 9, 1 | PSD side 3: 11, 2, 6, 3, 10, 5 | 1x1 PSD: 8.
    p = 2, m = 3; column of variable 7 is empty, inequality row 1 is empty, c[2] = 0.  Variable 6 has four entries, equality
    row 0 has six."""
    rng = np.random.default_rng(103)
    n, p, m = 12, 2, 3
    psd = [np.array([11, 2, 6, 3, 10, 5]), np.array([8])]
    soc = [np.array([4, 9, 1])]
    ent_A = [(0, 11), (0, 6), (0, 3), (0, 4), (0, 0), (0, 8), (1, 6), (1, 2), (1, 9)]
    ent_G = [(0, 6), (0, 5), (0, 1), (2, 6), (2, 10), (2, 8), (2, 0)]
    A = _csc([r for r, _ in ent_A], [c for _, c in ent_A], rng.standard_normal(len(ent_A)), (p, n))
    G = _csc([r for r, _ in ent_G], [c for _, c in ent_G], rng.standard_normal(len(ent_G)), (m, n))
    c = rng.standard_normal(n)
    c[2] = 0.0
    return P.Problem(n=n, A=A, b=rng.standard_normal(p), G=G, h=rng.standard_normal(m), c=c, psd=psd, soc=soc, name="mixed")


def case_mixed(zero_c=False):
    pr = _mixed_problem()
    rng = np.random.default_rng(106)                         # (an iterate for which the four-term sums round differently backwards)
    x, y = _iterate(rng, pr.n, pr.p + pr.m)
    order = B.host_preprocess(pr, index_base=1)[0]
    return Case("mixed_zero_c" if zero_c else "mixed", pr, x, y, zero_c=zero_c, index_base=1,
                long_col=int(np.where(order == 6)[0][0]), long_row=0)


def case_grid_tail():
    """PSD side 22 (253 variables) and 4 free ones: n = 257, one more than a workgroup; Q = 257 rows (p = 129, m = 128).
    Column of variable 40 and row 200 hold 300 entries each: every row / column once and 43 of them twice."""
    rng = np.random.default_rng(105)
    n, p, m = 257, 129, 128
    Q = p + m
    rows, cols = [], []
    for r in range(Q):                                       # a sparse background: three entries per row
        for cc in rng.choice(n, 3, replace=False):
            rows.append(r); cols.append(int(cc))
    keep = [(r, cc) for r, cc in zip(rows, cols) if cc != 40 and r != 200]
    rows, cols = [r for r, _ in keep], [cc for _, cc in keep]
    rows += list(range(Q)) + list(range(43)); cols += [40] * 300
    rows += [200] * 299; cols += [cc for cc in range(n) if cc != 40] + list(range(41, 41 + 43))
    vals = rng.standard_normal(len(rows))
    rows, cols = np.array(rows), np.array(cols)
    ea = rows < p
    A = _csc(rows[ea], cols[ea], vals[ea], (p, n))
    G = _csc(rows[~ea] - p, cols[~ea], vals[~ea], (m, n))
    pr = P.Problem(n=n, A=A, b=rng.standard_normal(p), G=G, h=rng.standard_normal(m), c=rng.standard_normal(n),
                   psd=[np.arange(253, dtype=np.int64)], name="grid-tail")
    x, y = _iterate(rng, n, Q)
    return Case("grid_tail", pr, x, y, long_col=40, long_row=200)


def case_dense():
    pr = P.randsdp(5, 4, seed=2, dense=True)
    rng = np.random.default_rng(106)
    x, y = np.zeros(pr.n), rng.standard_normal(pr.p + pr.m)
    x[9] = 0.25                                              # (entry (3, 3) of the block: a diagonal one)
    y[:pr.p] = 0.0
    y[2] = -4.0
    return Case("dense", pr, x, y)


def all_cases():
    return [case_one_equality(), case_one_inequality(), case_mixed(), case_grid_tail(), case_dense(), case_mixed(zero_c=True)]


def solver_layout(case):
    """(order, inv, offdiag, blocks [(offset, side)], socs [(offset, len)], conelen) of the solver's variable order"""
    pr = case.prob
    order, inv = B.host_preprocess(pr, index_base=case.index_base)[:2]
    offdiag = np.zeros(pr.n, dtype=bool)
    blocks, socs, pos = [], [], 0
    for side in B.psd_sides(pr):
        blocks.append((pos, side))
        for j in range(side):
            for i in range(j + 1):
                offdiag[pos] = i != j
                pos += 1
    for s in pr.soc:
        socs.append((pos, len(s)))
        pos += len(s)
    return order, inv, offdiag, blocks, socs, pos


def stacked(case):
    """M = [A; G] as the library receives it (sorted CSC, duplicates kept), a dense A as stored rows"""
    pr = case.prob
    A = sp.csc_matrix(pr.A, dtype=np.float64)
    G = sp.csc_matrix(pr.G, dtype=np.float64)
    A.sort_indices(); G.sort_indices()
    return A, G


def expected(case, reverse_col=None, reverse_row=None):
    pr = case.prob
    n, p, m = pr.n, pr.p, pr.m
    order, inv, offdiag, blocks, socs, conelen = solver_layout(case)
    A, G = stacked(case)
    dense = getattr(pr, "M_dense", None)
    inv_sqrt2 = 1.0 / math.sqrt(2.0)
    x = [float(v) * inv_sqrt2 if offdiag[k] else float(v) for k, v in enumerate(case.x)]
    y = [float(v) for v in case.y]
    c = [0.0 if case.zero_c else float(pr.c[order[k]]) for k in range(n)]
    bh = [float(v) for v in pr.b] + [float(v) for v in pr.h]
    # column k of M in storage order: A's entries of variable order[k], then G's (rows offset by p)
    col_entries = []
    for k in range(n):
        j = int(order[k])
        ent = [] if dense is not None else [(int(A.indices[q]), float(A.data[q])) for q in range(A.indptr[j], A.indptr[j + 1])]
        ent += [(int(G.indices[q]) + p, float(G.data[q])) for q in range(G.indptr[j], G.indptr[j + 1])]
        col_entries.append(ent)
    row_entries = [[] for _ in range(p + m)]
    for k in range(n):
        for r, v in col_entries[k]:
            row_entries[r].append((k, v))
    slack = []
    for r in range(p + m):
        acc = 0.0
        if dense is not None and r < p:                      # (exact: x has one non-zero entry, a power of two)
            acc = float(sum(float(dense[r, k]) * x[k] for k in range(n)))
        ent = row_entries[r][::-1] if r == reverse_row else row_entries[r]
        for k, v in ent:
            acc = acc + v * x[k]
        slack.append(acc - bh[r])
    dc = []
    for k in range(n):
        base = c[k]
        if dense is not None:                                # c + A'y (exact product: y_eq has one non-zero entry)
            base = float(sum(float(dense[r, k]) * y[r] for r in range(p))) + c[k]
        acc = 0.0
        ent = col_entries[k][::-1] if k == reverse_col else col_entries[k]
        for r, v in ent:
            acc = acc + v * y[r]
        v = base + acc
        if offdiag[k]:
            v = v / 2.0
        dc.append(v)
    ineq = -min(0.0, min(y[p:])) if m > 0 else 0.0
    ones = [dc[off] for off, side in blocks if side == 1]
    one_viol = max(0.0, -min(0.0, min(ones))) if ones else 0.0
    margins = []
    for off, ln in socs:
        ss = 0.0
        for i in range(1, ln):
            ss = ss + dc[off + i] * dc[off + i]
        margins.append(dc[off] - math.sqrt(ss))
    soc_viol = max(0.0, -min(0.0, min(margins))) if margins else 0.0
    zero_viol = max([0.0] + [abs(v) for v in dc[conelen:]])
    neg = []
    for off, side in blocks:
        if side >= 2:
            neg += [-v for v in dc[off:off + side * (side + 1) // 2]]
    return dict(primal=np.array([x[inv[i]] for i in range(n)]), dual_cone=np.array([dc[inv[i]] for i in range(n)]),
                dual_eq=np.array(y[:p]), dual_in=np.array(y[p:]), slack_eq=np.array(slack[:p]), slack_in=np.array(slack[p:]),
                viol=np.array([ineq, one_viol, soc_viol, zero_viol]), neg=np.array(neg))


KEYS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in", "viol", "neg")


def same_bits(a, b):
    """equal as bit patterns (so that -0.0 and 0.0 differ and NaN equals NaN)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
