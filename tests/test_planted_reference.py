"""The closed-form planted reference of helpers.ClosedFormPlanted (the large-side GPU tests' oracle) against the dense
NumPy construction of the same matrix.  CPU only."""
import numpy as np
import pytest

from helpers import ClosedFormPlanted, packed_symv_ref, smat, svec

SIDES = [1, 2, 3, 63, 64, 65, 130, 257]
TOP = [50.0, 20.0, 7.0, 4.0, 2.5]


def _dense(P):
    n = P.n
    H = [np.eye(n) - 2.0 * np.outer(P.U[:, k], P.U[:, k]) for k in (0, 1)]
    return H[0] @ H[1]


def _close(a, b, rel=1e-14):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("n", SIDES)
def test_closed_form_matches_dense_construction(n):
    P = ClosedFormPlanted(n, 100 + n, TOP, bulk=(-3.0, 0.5))
    Q = _dense(P)
    X = (Q * P.lam) @ Q.T
    # the planted values, unsorted on the diagonal of D
    k = min(len(TOP), n)
    assert np.array_equal(P.sorted_vals()[:k], np.sort(TOP[:k])[::-1])
    assert np.array_equal(P.sorted_vals(), np.sort(P.lam)[::-1])
    if n >= 64:
        assert not np.all(np.diff(P.lam) <= 0)
    # packed entries
    x = P.fill_packed()
    assert _close(x, svec(X))
    # X v, one vector and a block of columns
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n)
    V = rng.standard_normal((n, 3))
    assert _close(P.matvec(v), X @ v)
    assert _close(P.matvec(V), X @ V)
    # eigenpairs: Q e_i, and they are eigenpairs of the dense X
    idx = P.order[:min(4, n)]
    lam, Z = P.eigpairs(idx)
    assert np.array_equal(lam, P.lam[idx])
    assert _close(Z, Q[:, idx])
    assert np.abs(X @ Z - Z * lam).max() <= 1e-13 * np.abs(P.lam).max()
    assert np.abs(Z.T @ Z - np.eye(len(idx))).max() <= 1e-14
    # the spectrum itself, against LAPACK on the dense matrix
    assert np.abs(np.linalg.eigvalsh(X)[::-1] - P.sorted_vals()).max() <= 1e-13 * np.abs(P.lam).max()
    # X+ and the top-r projection
    Xp = (Q * np.maximum(P.lam, 0.0)) @ Q.T
    assert _close(P.fill_packed(d=P.d_plus()), svec(Xp))
    r = min(3, n)
    lt, Zt = P.top(r)
    assert _close(P.fill_packed(d=P.d_top(r)), svec((Zt * lt) @ Zt.T))
    assert _close(P.fill_packed(d=P.d_top(r)), svec((Q[:, P.order[:r]] * lt) @ Q[:, P.order[:r]].T))
    # the operator bound covers the rounding of the packed matrix
    assert np.linalg.norm(smat(x, n) - X, 2) <= P.op_err()


@pytest.mark.parametrize("n", SIDES)
def test_packed_bits_do_not_depend_on_chunk_size(n):
    P = ClosedFormPlanted(n, 7 + n, TOP, bulk=(-1.0, 1.0))
    for d in (None, P.d_plus(), P.d_top(min(2, n))):
        a = P.fill_packed(d=d, chunk_entries=1)              # one column per chunk
        b = P.fill_packed(d=d, chunk_entries=5 * n + 3)
        c = P.fill_packed(d=d, chunk_entries=1 << 24)        # one chunk
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # chunks cover the packed array exactly once, in order
    N = n * (n + 1) // 2
    spans = [(a, b) for a, b, _ in P.chunks(chunk_entries=3 * n)]
    assert spans[0][0] == 0 and spans[-1][1] == N and all(p[1] == q[0] for p, q in zip(spans, spans[1:]))


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_chunked_symv_reference(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n * (n + 1) // 2)
    v = rng.standard_normal(n)
    X = smat(x, n)
    for ch in (1, 4 * n + 1, 1 << 24):
        y, b = packed_symv_ref(x, n, v, chunk_entries=ch)
        assert _close(y, X @ v, 1e-13)
        assert np.allclose(b, np.abs(X) @ np.abs(v), rtol=1e-13, atol=0)
