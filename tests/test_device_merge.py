"""The rank-one merge of the split K x K eigensolve on the device (csrc/merge_device.hip.hpp, options.device_eig_merge),
through proxsdp_device_symeig_split -- the code the Lanczos driver runs -- against LAPACK and the host merge, whose bits
it reproduces."""
import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

from device_merge_cases import KS, cases, rayleigh_quotient

pytestmark = pytest.mark.gpu


def _check(name, K, D, f, al, be, k1):
    """the host merge's own bounds (test_split_and_rank_one_merge_eigensolver_against_lapack): same method, same error sources"""
    T = rayleigh_quotient(D, f, al, be)
    d, U, info = B.device_symeig_split(D, f, al, be, k1)
    sc = max(1.0, np.abs(T).max())
    e_val = np.abs(d - np.linalg.eigvalsh(T)).max()
    e_orth = np.abs(U.T @ U - np.eye(K)).max()
    e_res = np.abs(T @ U - U * d).max()
    print(name, K, "eigenvalues %.2e orthogonality %.2e residual %.2e bound %.2e" % (e_val, e_orth, e_res, 1e-13 * K * sc), info)
    assert e_val <= 1e-13 * K * sc, name
    assert e_orth <= 1e-13, name
    assert e_res <= 1e-13 * K * sc, name
    assert np.all(np.diff(d) >= 0), name
    # the host merge on the same input: the planner is shared, so the two kinds of pole split identically
    dh, Uh, infoh = B.host_symeig_split(D, f, al, be, k1)
    assert info["nondeflated"] == infoh["nondeflated"] and info["deflated"] == infoh["deflated"], (name, info, infoh)
    assert info["nondeflated"] + info["deflated"] == K
    assert np.abs(d - dh).max() <= 1e-13 * K * sc, name
    assert info["max_secular_iterations"] <= 40, (name, info)
    # more than the bound: the device runs every sum in the host's order -- the same bits, eigenvectors included
    assert np.array_equal(d, dh) and np.array_equal(U, Uh) and info == infoh, name
    # fixed-order reductions: a second run gives the same bits
    d2, U2, info2 = B.device_symeig_split(D, f, al, be, k1)
    assert np.array_equal(d, d2) and np.array_equal(U, U2) and info == info2, name
    return info


@pytest.mark.parametrize("K", KS)
def test_device_merge_against_lapack_and_the_host_merge(K):
    for name, D, f, al, be, k1 in cases(K):
        info = _check(name, K, D, f, al, be, k1)
        if name == "decoupled":
            assert info["nondeflated"] == 0


def test_device_merge_with_a_one_by_one_tail():
    """K = 5 split at k1 = 4: k2 = 1"""
    name, D, f, al, be, _ = cases(5)[0]
    _check(name + " k2=1", 5, D, f, al, be, 4)
