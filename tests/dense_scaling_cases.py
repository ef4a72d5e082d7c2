"""Instances shared by the dense-A equilibration / sigma_max tests (host and GPU)."""
import numpy as np
import scipy.sparse as sp

from oracle import Options
from oracle import pdhg as opdhg
from proxsdp_jl_amd import problems as P


def inst_a():
    return P.randsdp(60, 40, seed=3, dense=True)


def inst_b():
    return P.randsdp(30, 20, seed=1, varbounds=False, dense=True)


def inst_c(dent=False):
    """PSD side 8, 6 dense rows uniform in [0.95, 1], no G, b = A svec(X) of a random PSD X: the only kind of M on
    which plain `equilibration = true` survives the reference's min/max test.  dent=True: one entry set to 0.5."""
    rng = np.random.default_rng(2)
    side, p = 8, 6
    N = side * (side + 1) // 2
    A = rng.uniform(0.95, 1.0, (p, N))
    Gm = rng.standard_normal((side, side))
    X = Gm @ Gm.T
    jj = np.repeat(np.arange(side), np.arange(1, side + 1))
    ii = np.arange(N) - jj * (jj + 1) // 2
    x = X[ii, jj]                                     # the triangle variables (the model's own scaling, as randsdp's b)
    c = rng.uniform(0.0, 1.0, N)
    if dent:
        A[2, 7] = 0.5
    b = A @ x
    return P.Problem(n=N, A=sp.csc_matrix((p, N)), b=b, G=sp.csc_matrix((0, N)), h=np.zeros(0), c=c,
                     psd=[np.arange(N, dtype=np.int64)], name="nearly-constant-n8-p6", M_dense=np.ascontiguousarray(A))


def as_sparse(pr):
    """The same numbers through the CSC entry."""
    return P.Problem(n=pr.n, A=sp.csc_matrix(np.asarray(pr.M_dense)), b=pr.b, G=pr.G, h=pr.h, c=pr.c, psd=pr.psd,
                     name=pr.name + "-csc")


def full_matrix(pr):
    """[A;G] as a dense array."""
    return np.vstack([np.asarray(pr.M_dense), pr.G.toarray()])


def offdiag_scale(pr):
    """s: sqrt(2)/2 on off-diagonal PSD columns (norm_scaling), 1 elsewhere; the variables are in cone order."""
    s = np.ones(pr.n)
    for idx in pr.psd:
        L = len(idx)
        side = int((np.sqrt(8 * L + 1) - 1) // 2)
        jj = np.repeat(np.arange(side), np.arange(1, side + 1))
        ii = np.arange(L) - jj * (jj + 1) // 2
        s[np.asarray(idx)[ii != jj]] = np.sqrt(2.0) / 2.0
    return s


class _Aff:
    def __init__(self, M, p, m):
        self.p, self.m, self.n = p, m, M.shape[1]


def oracle_scaling(pr, aliasing):
    """oracle.pdhg.equilibrate on [A;G] of `pr`: (E, D)."""
    M = full_matrix(pr)
    o = Options()
    o.equilibration_reference_aliasing = bool(aliasing)
    return opdhg.equilibrate(sp.csc_matrix(M), _Aff(M, pr.p, pr.m), o)
