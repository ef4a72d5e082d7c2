"""Inputs shared by the device-merge tests: the cases of test_split_and_rank_one_merge_eigensolver_against_lapack
(tests/test_host_abi.py), generated the same way, at the same sizes."""
import numpy as np

KS = [5, 9, 25, 53, 97, 127, 190, 255]


def rayleigh_quotient(D, f, al, be):
    """the restarted Rayleigh quotient [diag(D) f; f' tridiag(al, be)], dense"""
    K, m = len(al), len(D)
    T = np.zeros((K, K))
    T[np.arange(m), np.arange(m)] = D
    if m:
        T[m, :m] = T[:m, m] = f
    for j in range(m, K):
        T[j, j] = al[j]
        if j + 1 < K:
            T[j, j + 1] = T[j + 1, j] = be[j]
    return T


def cases(K):
    """(name, D, f, al, be, k1): plain tridiagonal, restarted quotient with converged and open pairs, repeated Ritz values,
    a vanishing coupling (everything deflates), a graded spectrum"""
    rng = np.random.default_rng(K)
    m = (3 * K) // 5
    out = []
    al = rng.standard_normal(K) * 3
    be = np.abs(1 + 0.3 * rng.standard_normal(K))
    out.append(("tridiagonal", np.zeros(0), np.zeros(0), al, be, K // 2))
    D = np.sort(rng.uniform(1, 60, m))[::-1].copy()
    f = rng.standard_normal(m) * np.where(np.arange(m) < m // 3, 1e-13, 1e-2)
    al2 = np.zeros(K); be2 = np.zeros(K)
    al2[m:] = rng.standard_normal(K - m)
    be2[m:] = np.abs(1 + 0.1 * rng.standard_normal(K - m))
    out.append(("restart", D, f, al2, be2, m + 1))
    D3 = D.copy(); D3[1] = D3[0]
    out.append(("repeated", D3, np.abs(f) + 1e-3, al2, be2, m + 1))
    be4 = be2.copy(); be4[m] = 1e-14
    out.append(("decoupled", D, f, al2, be4, m + 1))
    out.append(("graded", np.zeros(0), np.zeros(0), np.geomspace(1e3, 1e-6, K), np.geomspace(1, 1e-8, K), K // 2))
    return out
